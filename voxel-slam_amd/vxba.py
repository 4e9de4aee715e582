"""ctypes binding of ``libvxba.so`` (include/vxba.h) with the reference's own names.

``LidarFactor`` mirrors ``class LidarFactor`` (VoxelSLAM/src/voxel_map.hpp:109-290) and
``Lidar_BA_Optimizer`` mirrors voxel_map.hpp:293-444, so parity tests read like calls into
the reference.  Everything numeric happens in the HIP kernels behind the C ABI; this module
holds no arithmetic and has NO CPU fallback -- a missing library or GPU raises ``VxbaError``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VXBA_LIB") or os.path.join(_HERE, "csrc", "libvxba.so")   # VXBA_LIB: A/B runs of two builds
MAX_WIN = 10
MAX_WIN_WIDE = 128
TRACE_COLS = 8

_f64p = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")
_i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
_ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p)
_HESS_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))
_RESID_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double))

# every symbol include/vxba.h declares (the CPU test suite checks the library exports all of them)
EXPORTS = [
    "vxba_create", "vxba_destroy", "vxba_clear", "vxba_set_win_size", "vxba_win_size", "vxba_size", "vxba_set_stream",
    "vxba_reserve", "vxba_last_error", "vxba_push_voxels", "vxba_push_points", "vxba_read_clusters", "vxba_acc_evaluate2",
    "vxba_evaluate_only_residual", "vxba_get_collective_time", "vxba_get_fused_time", "vxba_debug_partials", "vxba_acc_evaluate2_device", "vxba_evaluate_only_residual_device", "vxba_packed_len",
    "vxba_read_cache", "vxba_snapshot_cache", "vxba_restore_cache", "vxba_plane_fit", "vxba_plane_fit_judge", "vxba_build_clusters", "vxba_set_allreduce",
    "vxba_rccl_unique_id", "vxba_rccl_attach", "vxba_rccl_attach_bcast", "vxba_rccl_detach", "vxba_peer_export", "vxba_peer_attach", "vxba_peer_detach", "vxba_peer_status", "vxba_peer_selftest", "vxba_use_external_buffers", "vxba_damping_iter", "vxba_damping_iter_generic", "vxba_lm_steps", "vxba_set_profiling", "vxba_get_kernel_times", "vxba_algorithmic_bytes", "vxba_nnz", "vxba_device_bytes", "vxba_debug_mfma_probe", "vxba_debug_stamps", "vxba_debug_band_schur", "vxba_debug_lm_solve", "vxba_debug_wide_solve", "vxba_debug_host_damped_step", "vxba_push_voxels_csr",
    "vxba_imu_init", "vxba_imu_add", "vxba_imu_evaluate", "vxba_imu_update_state", "vxba_hess_plus", "vxba_hess_plus_gravity", "vxba_li_evaluate", "vxba_li_evaluate_gravity",
    "vxba_li_only_residual", "vxba_li_damping_iter", "vxba_imu_evaluate_g", "vxba_li_damping_iter_gravity", "vxba_voxelize_push", "vxba_set_precision",
    "vxba_lio_create", "vxba_lio_destroy", "vxba_lio_last_error", "vxba_lio_map_update", "vxba_lio_map_clear", "vxba_lio_map_size", "vxba_lio_scan_raw",
    "vxba_lio_scan_set", "vxba_lio_scan_size", "vxba_lio_scan_read", "vxba_lio_sweep", "vxba_lio_state_estimation", "vxba_lio_pvec_update", "vxba_lio_leaf_stats", "vxba_cov_add_build", "vxba_plane_update", "vxba_down_sampling_voxel", "vxba_voxelize_push_device",
    "vxba_set_option", "vxba_get_option", "vxba_lio_set_option",
    "vxba_hba_create", "vxba_hba_destroy", "vxba_hba_last_error", "vxba_hba_add_keyframes", "vxba_hba_num_keyframes", "vxba_hba_threads_used", "vxba_hba_clear", "vxba_hba_pass", "vxba_hba_num_windows", "vxba_hba_window", "vxba_hba_bottom", "vxba_hba_export_submaps", "vxba_hba_import_submaps", "vxba_hba_top_factor", "vxba_hba_top", "vxba_voxelize_profile",
    "vxba_map_create", "vxba_map_destroy", "vxba_map_last_error", "vxba_map_cut_voxel", "vxba_map_cut_voxel_device", "vxba_map_cut_voxel_fix", "vxba_map_cut_voxel_fix_device",
    "vxba_map_clear", "vxba_map_loop_update", "vxba_map_recut", "vxba_map_margi",
    "vxba_pgo_create", "vxba_pgo_destroy", "vxba_pgo_last_error", "vxba_pgo_clear", "vxba_pgo_num_nodes", "vxba_pgo_num_factors", "vxba_pgo_set_poses", "vxba_pgo_read_poses",
    "vxba_pgo_add_edges", "vxba_pgo_add_priors", "vxba_pgo_cost", "vxba_pgo_optimize", "vxba_pgo_stats",
    "vxba_loopreg_create", "vxba_loopreg_destroy", "vxba_loopreg_last_error", "vxba_loopreg_clear", "vxba_loopreg_num_clouds", "vxba_loopreg_cloud_size", "vxba_loopreg_read_cloud",
    "vxba_loopreg_stats", "vxba_loopreg_add_cloud", "vxba_loopreg_add_keyframe", "vxba_loopreg_associate", "vxba_loopreg_score", "vxba_loopreg_icp",
    "vxba_loopsearch_create", "vxba_loopsearch_destroy", "vxba_loopsearch_last_error", "vxba_loopsearch_clear", "vxba_loopsearch_num_frames", "vxba_loopsearch_num_descriptors",
    "vxba_loopsearch_default_params", "vxba_loopsearch_describe", "vxba_loopsearch_read_descriptors", "vxba_loopsearch_search", "vxba_loopsearch_read_matches", "vxba_loopsearch_add",
    "vxba_loopsearch_stats", "vxba_loopsearch_search_multi", "vxba_loopsearch_read_match_offsets",
    "vxba_map_set_plane_thresholds",
    "vxba_init_pose_table", "vxba_init_deskew", "vxba_init_normal_scatter", "vxba_imu_push", "vxba_init_motion", "vxba_init_motion_times", "vxba_down_sampling_close",
    "vxba_initodom_create", "vxba_initodom_destroy", "vxba_initodom_last_error", "vxba_initodom_clear", "vxba_initodom_cloud_size", "vxba_initodom_cloud",
    "vxba_initodom_search", "vxba_initodom_step", "vxba_initodom_inspect", "vxba_initodom_stats",
    "vxba_keyframe_create", "vxba_keyframe_destroy", "vxba_keyframe_last_error", "vxba_keyframe_clear", "vxba_keyframe_push_scan", "vxba_keyframe_push_scan_device", "vxba_keyframe_info",
    "vxba_keyframe_read", "vxba_keyframe_device", "vxba_keyframe_device_down_xyz", "vxba_keyframe_num_scans", "vxba_keyframe_num_buffered", "vxba_keyframe_scan_poses", "vxba_keyframe_stats", "vxba_keyframe_set_profiling", "vxba_keyframe_stage_times",
    "vxba_loopreg_add_keyframe_device", "vxba_hba_add_keyframes_device",
    "vxba_corner_default_params", "vxba_corner_create", "vxba_corner_destroy", "vxba_corner_last_error", "vxba_corner_extract", "vxba_corner_extract_device",
    "vxba_corner_extract_with_planes", "vxba_corner_read", "vxba_corner_planes", "vxba_corner_projection_planes", "vxba_corner_candidates", "vxba_corner_stats",
    "vxba_corner_set_profiling", "vxba_corner_stage_times",
    "vxba_imuekf_default_params", "vxba_imuekf_create", "vxba_imuekf_destroy", "vxba_imuekf_last_error", "vxba_imuekf_process", "vxba_imuekf_read_scan", "vxba_imuekf_pose_table",
    "vxba_imuekf_reinit", "vxba_imuekf_clear", "vxba_imuekf_filter", "vxba_imuekf_filter_passes", "vxba_imuekf_filtered", "vxba_imuekf_filtered_device", "vxba_imuekf_stats",
    "vxba_imuekf_set_profiling", "vxba_imuekf_stage_times",
    "vxba_lio_scan_raw_device",
    "vxba_intake_create", "vxba_intake_destroy", "vxba_intake_last_error", "vxba_intake_push", "vxba_intake_read", "vxba_intake_device", "vxba_intake_stats",
    "vxba_intake_set_profiling", "vxba_intake_stage_times", "vxba_imuekf_process_device", "vxba_intake_push_yaw", "vxba_intake_yaw_info",
    "vxba_session_create", "vxba_session_destroy", "vxba_session_last_error", "vxba_session_clear", "vxba_session_load_scans", "vxba_session_num_scans",
    "vxba_session_build_keyframes", "vxba_session_num_keyframes", "vxba_session_keyframes", "vxba_session_read_keyframes", "vxba_session_device",
    "vxba_session_set_scan_poses", "vxba_session_num_windows", "vxba_session_window_cloud", "vxba_session_read_window", "vxba_session_stats",
    "vxba_session_set_profiling", "vxba_session_stage_times",
    "vxba_globalmap", "vxba_hba_device_clouds",
    "vxba_map_loop_update_device", "vxba_map_scan_device",
    "vxba_kfarchive_create", "vxba_kfarchive_destroy", "vxba_kfarchive_last_error", "vxba_kfarchive_clear", "vxba_kfarchive_add", "vxba_kfarchive_add_device", "vxba_kfarchive_num",
    "vxba_kfarchive_info", "vxba_kfarchive_read", "vxba_kfarchive_device", "vxba_kfarchive_set_poses", "vxba_kfarchive_arm_history", "vxba_kfarchive_history_size",
    "vxba_kfarchive_load_near", "vxba_kfarchive_map_loop", "vxba_kfarchive_map_loop_scans", "vxba_kfarchive_stats",
    "vxba_map_slide", "vxba_map_counts", "vxba_map_fix_pool", "vxba_map_set_journey", "vxba_map_release", "vxba_map_device_bytes", "vxba_map_leaves", "vxba_map_leaf_points", "vxba_map_cut_voxel_lio", "vxba_map_export_planes",
]

_ERRNAMES = {1: "VXBA_ERR_ARG", 2: "VXBA_ERR_HIP", 3: "VXBA_ERR_NODEV", 4: "VXBA_ERR_STATE", 5: "VXBA_ERR_UNSUPPORTED"}


class VxbaError(RuntimeError):
    pass


class VoxelizeParams(C.Structure):
    """vxba_voxelize_params: the knobs of OctreeGBA::recut (loop_refine.hpp:311-315, 358-378) and of the voxel grid."""
    _fields_ = [("voxel_size", C.c_double), ("max_layer", C.c_int), ("min_points", C.c_int), ("min_eigen_value", C.c_double),
                ("eigen_ratio", C.c_double * 4), ("factor_ratio_max", C.c_double), ("min_points_layer", C.c_int * 4), ("min_frames", C.c_int),
                ("shard_index", C.c_int), ("shard_count", C.c_int)]

    def __init__(self, voxel_size=1.0, max_layer=2, min_points=10, min_eigen_value=0.01, eigen_ratio=(1 / 16, 1 / 16, 1 / 16, 1 / 16),
                 factor_ratio_max=0.12, min_points_layer=(0, 0, 0, 0), min_frames=2, shard_index=0, shard_count=0):
        """Defaults: OctreeGBA.  OctoTree's batch build (motion_init): min_points_layer=min_point[layer], min_frames=0.
        shard_count > 1: keep the root voxels that hash to shard_index (voxel-sharded windows, one rank per GPU)."""
        super().__init__(voxel_size, max_layer, min_points, min_eigen_value, (C.c_double * 4)(*eigen_ratio), factor_ratio_max,
                         (C.c_int * 4)(*min_points_layer), min_frames, shard_index, shard_count)

    def sharded(self, shard_index: int, shard_count: int) -> "VoxelizeParams":
        """The same parameters for one shard of a voxel-sharded window."""
        return VoxelizeParams(self.voxel_size, self.max_layer, self.min_points, self.min_eigen_value, tuple(self.eigen_ratio), self.factor_ratio_max,
                              tuple(self.min_points_layer), self.min_frames, shard_index, shard_count)

    def as_array(self):
        return np.array([self.voxel_size, self.max_layer, self.min_points, self.min_eigen_value, *self.eigen_ratio, self.factor_ratio_max,
                         *self.min_points_layer, self.min_frames], dtype=np.float64)


_lib = None


class InitMotionParams(C.Structure):
    """``vxba_init_motion_params`` of include/vxba.h."""
    _fields_ = [("imupre_scale_gravity", C.c_double), ("dept_err", C.c_double), ("beam_err", C.c_double), ("imu_coef", C.c_double),
                ("noise_meas", C.c_double * 36), ("noise_walk", C.c_double * 36), ("min_eigen_value", C.c_double), ("plane_eigen_value_thre", C.c_double * 4),
                ("point_notime", C.c_int)]


class ImuEkfParams(C.Structure):
    """``vxba_imuekf_params``: the four noise 3-vectors of ``IMUEKF``, the extrinsic [R 9 column-major | p 3], ``acc_in_g`` (upstream's
    ``imu_topic == "/livox/imu"``) and ``point_notime``."""
    _fields_ = [("cov_acc", C.c_double * 3), ("cov_gyr", C.c_double * 3), ("cov_bias_gyr", C.c_double * 3), ("cov_bias_acc", C.c_double * 3),
                ("ext", C.c_double * 12), ("acc_in_g", C.c_int), ("point_notime", C.c_int)]

    @classmethod
    def make(cls, cov_acc=0.1, cov_gyr=0.1, cov_bias_gyr=1e-4, cov_bias_acc=1e-4, ext=None, acc_in_g=True, point_notime=False):
        p = cls()
        for name, v in (("cov_acc", cov_acc), ("cov_gyr", cov_gyr), ("cov_bias_gyr", cov_bias_gyr), ("cov_bias_acc", cov_bias_acc)):
            setattr(p, name, (C.c_double * 3)(*np.broadcast_to(np.asarray(v, dtype=np.float64), (3,))))
        e = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]) if ext is None else np.asarray(ext, dtype=np.float64).reshape(12)
        p.ext = (C.c_double * 12)(*e)
        p.acc_in_g, p.point_notime = int(bool(acc_in_g)), int(bool(point_notime))
        return p


class ScanLayout(C.Structure):
    """``vxba_scan_layout``: where x, y, z (float32) and the time field sit in one point of a driver message, and what becomes of the time.
    ``time_type``: TIME_*; ``time_rule``: RULE_* (``RULE_YAW``: the times come from the yaw angles, :meth:`ScanIntake.push_yaw`); ``filter`` 0: every point
    is taken (TartanAir)."""
    _fields_ = [("point_step", C.c_int32), ("off_x", C.c_int32), ("off_y", C.c_int32), ("off_z", C.c_int32), ("off_time", C.c_int32), ("time_type", C.c_int32),
                ("time_rule", C.c_int32), ("filter", C.c_int32)]
    TIME_NONE, TIME_F32, TIME_U32, TIME_F64 = 0, 1, 2, 3
    RULE_NONE, RULE_AS_IS, RULE_NANOSECONDS, RULE_MINUS_HEAD, RULE_YAW = 0, 1, 2, 3, 4
    MAX_STEP = 240
    TIME_DTYPES = {0: None, 1: "<f4", 2: "<u4", 3: "<f8"}

    def as_tuple(self):
        return tuple(int(getattr(self, f)) for f, _ in self._fields_)


class MapParams(C.Structure):
    """vxba_map_params (include/vxba.h)."""
    _fields_ = [("voxel_size", C.c_double), ("max_layer", C.c_int), ("min_point", C.c_double * 4), ("min_eigen_value", C.c_double),
                ("plane_eigen_value_thre", C.c_double * 4), ("max_points", C.c_int), ("win_size", C.c_int), ("thread_num", C.c_int)]


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load libvxba.so; fails loudly if it has not been built (``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise VxbaError(f"{path} not found: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()')")
    L = C.CDLL(path)
    vp, ci, cd = C.c_void_p, C.c_int, C.c_double
    L.vxba_create.argtypes = [ci, ci, C.POINTER(vp)]
    L.vxba_destroy.argtypes = [vp]
    L.vxba_clear.argtypes = [vp]
    L.vxba_set_win_size.argtypes = [vp, ci]
    L.vxba_win_size.argtypes = [vp]
    L.vxba_size.argtypes = [vp]
    L.vxba_set_stream.argtypes = [vp, vp]
    L.vxba_reserve.argtypes = [vp, ci]
    L.vxba_last_error.argtypes = [vp]
    L.vxba_last_error.restype = C.c_char_p
    L.vxba_push_voxels.argtypes = [vp, ci, _f64p, _f64p, _f64p, vp, vp, vp]
    L.vxba_push_voxels_csr.argtypes = [vp, ci, vp, vp, vp, _f64p, _f64p, vp, vp, vp]
    L.vxba_push_points.argtypes = [vp, ci, C.c_int64, _f64p, _i64p, vp, vp]
    L.vxba_read_clusters.argtypes = [vp, ci, ci, _f64p]
    L.vxba_acc_evaluate2.argtypes = [vp, _f64p, ci, ci, _f64p, _f64p, C.POINTER(cd)]
    L.vxba_evaluate_only_residual.argtypes = [vp, _f64p, ci, ci, C.POINTER(cd)]
    L.vxba_acc_evaluate2_device.argtypes = [vp, _f64p, ci, ci, vp]
    L.vxba_evaluate_only_residual_device.argtypes = [vp, _f64p, ci, ci, vp]
    L.vxba_packed_len.argtypes = [vp]
    L.vxba_packed_len.restype = C.c_size_t
    L.vxba_read_cache.argtypes = [vp, ci, ci, _f64p, _f64p, _f64p]
    L.vxba_snapshot_cache.argtypes = [vp]
    L.vxba_restore_cache.argtypes = [vp]
    L.vxba_plane_fit.argtypes = [ci, C.c_int64, _f64p, _f64p, _f64p]
    L.vxba_plane_fit_judge.argtypes = [ci, C.c_int64, _f64p, ci, cd, cd, cd, _f64p, _f64p, np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")]
    L.vxba_build_clusters.argtypes = [ci, C.c_int64, C.c_int64, _f64p, _i64p, _f64p]
    L.vxba_set_allreduce.argtypes = [vp, _ALLREDUCE_FN, vp]
    L.vxba_use_external_buffers.argtypes = [vp, vp, vp]
    L.vxba_rccl_unique_id.argtypes = [C.c_char_p, vp]
    L.vxba_rccl_attach.argtypes = [vp, C.c_char_p, ci, ci, vp]
    L.vxba_rccl_detach.argtypes = [vp]
    L.vxba_damping_iter.argtypes = [vp, _f64p, ci, _f64p, _f64p, _f64p, C.POINTER(ci), C.POINTER(ci)]
    L.vxba_damping_iter_generic.argtypes = [ci, _f64p, ci, _HESS_FN, _RESID_FN, vp, _f64p, _f64p, _f64p, C.POINTER(ci), C.POINTER(ci)]
    L.vxba_lm_steps.argtypes = [vp, _f64p, ci, ci, _f64p, _f64p, _i64p]
    L.vxba_set_profiling.argtypes = [vp, ci]
    L.vxba_set_precision.argtypes = [vp, ci]
    L.vxba_get_kernel_times.argtypes = [vp, _f64p, _i64p, ci]
    L.vxba_get_collective_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), ci]
    L.vxba_get_fused_time.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64), ci]
    L.vxba_algorithmic_bytes.argtypes = [vp, _f64p]
    L.vxba_nnz.argtypes = [vp, C.POINTER(C.c_int64)]
    L.vxba_device_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.vxba_debug_mfma_probe.argtypes = [ci, _f64p, _f64p, _f64p]
    L.vxba_debug_stamps.argtypes = [ci, vp, C.c_size_t]
    L.vxba_debug_lm_solve.argtypes = [ci, ci, _f64p, _f64p, cd, vp, ci, ci, vp, C.c_uint, _f64p, _f64p, C.POINTER(cd), vp]
    L.vxba_debug_wide_solve.argtypes = [ci, ci, _f64p, cd, ci, _f64p, _f64p, _f64p, C.POINTER(ci)]
    L.vxba_debug_host_damped_step.argtypes = [ci, _f64p, _f64p, cd, _f64p, _f64p, _f64p, C.POINTER(cd)]
    L.vxba_imu_init.argtypes = [_f64p, vp, vp]
    L.vxba_imu_add.argtypes = [_f64p, _f64p, _f64p, cd, _f64p, _f64p]
    L.vxba_imu_evaluate.argtypes = [_f64p, _f64p, _f64p, ci, vp, vp, C.POINTER(cd)]
    L.vxba_imu_update_state.argtypes = [_f64p, _f64p]
    L.vxba_hess_plus.argtypes = [ci, _f64p, _f64p, _f64p, _f64p]
    L.vxba_li_evaluate.argtypes = [vp, _f64p, _f64p, cd, _f64p, _f64p, C.POINTER(cd)]
    L.vxba_hess_plus_gravity.argtypes = [ci, _f64p, _f64p, _f64p, _f64p]
    L.vxba_li_evaluate_gravity.argtypes = [vp, _f64p, _f64p, cd, _f64p, _f64p, C.POINTER(cd)]
    L.vxba_li_only_residual.argtypes = [vp, _f64p, _f64p, cd, C.POINTER(cd)]
    L.vxba_li_damping_iter.argtypes = [vp, _f64p, _f64p, cd, ci, vp, vp, C.POINTER(ci)]
    L.vxba_voxelize_push.argtypes = [vp, C.c_int64, _f64p, _i64p, _f64p, C.POINTER(VoxelizeParams), C.POINTER(C.c_int64), vp, C.c_int64]
    L.vxba_voxelize_push_device.argtypes = [vp, C.c_int64, vp, _i64p, _f64p, C.POINTER(VoxelizeParams), C.POINTER(C.c_int64), vp, C.c_int64]
    L.vxba_imu_evaluate_g.argtypes = [_f64p, _f64p, _f64p, ci, vp, vp, C.POINTER(cd)]
    L.vxba_li_damping_iter_gravity.argtypes = [vp, _f64p, _f64p, cd, ci, vp, _f64p, vp, C.POINTER(ci)]
    i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
    L.vxba_lio_create.argtypes = [cd, ci, ci, C.POINTER(vp)]
    L.vxba_lio_destroy.argtypes = [vp]
    L.vxba_lio_last_error.argtypes = [vp]
    L.vxba_lio_last_error.restype = C.c_char_p
    L.vxba_lio_map_update.argtypes = [vp, C.c_int64, _i64p, i32p, i32p, vp, _f64p, _f64p, _f64p, _f64p]
    L.vxba_lio_map_clear.argtypes = [vp]
    L.vxba_lio_map_size.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.vxba_lio_scan_raw.argtypes = [vp, C.c_int64, np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS"), vp, cd, cd]
    L.vxba_lio_scan_set.argtypes = [vp, C.c_int64, _f64p, _f64p]
    L.vxba_lio_scan_size.argtypes = [vp]
    L.vxba_lio_scan_size.restype = C.c_int64
    L.vxba_lio_scan_read.argtypes = [vp, _f64p, _f64p]
    L.vxba_lio_sweep.argtypes = [vp, _f64p, _f64p, ci, _f64p, vp, vp]
    L.vxba_lio_state_estimation.argtypes = [vp, _f64p, _f64p, vp, vp]
    L.vxba_lio_pvec_update.argtypes = [vp, _f64p, _f64p, vp, vp]
    L.vxba_lio_leaf_stats.argtypes = [vp, C.c_int64, _i64p, vp, _f64p, _f64p]
    L.vxba_cov_add_build.argtypes = [ci, C.c_int64, C.c_int64, _f64p, _f64p, _i64p, _f64p]
    L.vxba_down_sampling_voxel.argtypes = [ci, C.c_int64, np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS"), cd,
                                           np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS"), C.POINTER(C.c_int64)]
    L.vxba_down_sampling_close.argtypes = [ci, C.c_int64, np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS"), cd,
                                           np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS"), i32p, C.POINTER(C.c_int64)]
    L.vxba_plane_update.argtypes = [ci, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p]
    L.vxba_peer_export.argtypes = [vp, vp]
    L.vxba_peer_attach.argtypes = [vp, ci, ci, vp]
    L.vxba_peer_detach.argtypes = [vp]
    L.vxba_peer_status.argtypes = [vp, C.POINTER(ci)]
    L.vxba_peer_selftest.argtypes = [vp, C.POINTER(ci)]
    L.vxba_set_option.argtypes = [vp, ci, ci]
    L.vxba_get_option.argtypes = [vp, ci, C.POINTER(ci)]
    L.vxba_lio_set_option.argtypes = [vp, ci, ci]
    L.vxba_map_create.argtypes = [C.POINTER(MapParams), ci, C.POINTER(vp)]
    L.vxba_map_destroy.argtypes = [vp]
    L.vxba_map_last_error.argtypes = [vp]
    L.vxba_map_last_error.restype = C.c_char_p
    L.vxba_map_cut_voxel.argtypes = [vp, ci, C.c_int64, _f64p, _f64p, _f64p]
    L.vxba_map_cut_voxel_device.argtypes = [vp, ci, C.c_int64, vp, vp, vp]
    L.vxba_map_cut_voxel_lio.argtypes = [vp, ci, vp]
    L.vxba_map_cut_voxel_fix.argtypes = [vp, C.c_int64, vp, vp, C.c_double]
    L.vxba_map_cut_voxel_fix_device.argtypes = [vp, C.c_int64, vp, vp, C.c_double]
    L.vxba_map_clear.argtypes = [vp]
    L.vxba_map_set_plane_thresholds.argtypes = [vp, cd, _f64p]
    L.vxba_map_loop_update.argtypes = [vp, ci, vp, vp, vp, C.c_double, ci, vp, vp, vp, vp, vp]
    L.vxba_map_export_planes.argtypes = [vp, vp, C.POINTER(C.c_int64)]
    L.vxba_map_recut.argtypes = [vp, ci, _f64p, vp, C.POINTER(C.c_int64)]
    L.vxba_map_margi.argtypes = [vp, ci, _f64p, vp]
    L.vxba_map_slide.argtypes = [vp, ci]
    L.vxba_map_counts.argtypes = [vp, _i64p]
    L.vxba_map_fix_pool.argtypes = [vp, _i64p]
    L.vxba_map_set_journey.argtypes = [vp, C.c_double]
    L.vxba_map_release.argtypes = [vp, C.c_double, ci, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.vxba_map_device_bytes.argtypes = [vp, _i64p]
    L.vxba_map_leaves.argtypes = [vp, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
    L.vxba_map_leaf_points.argtypes = [vp, C.c_uint64, ci, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.vxba_pgo_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_pgo_destroy.argtypes = [vp]
    L.vxba_pgo_last_error.argtypes = [vp]
    L.vxba_pgo_last_error.restype = C.c_char_p
    L.vxba_pgo_clear.argtypes = [vp]
    L.vxba_pgo_num_nodes.argtypes = [vp]
    L.vxba_pgo_num_factors.argtypes = [vp]
    L.vxba_pgo_num_factors.restype = C.c_int64
    L.vxba_pgo_set_poses.argtypes = [vp, ci, _f64p]
    L.vxba_pgo_read_poses.argtypes = [vp, _f64p]
    L.vxba_pgo_add_edges.argtypes = [vp, C.c_int64, ci, ci, i32p, _f64p]
    L.vxba_pgo_add_priors.argtypes = [vp, C.c_int64, i32p, _f64p, _f64p]
    L.vxba_pgo_cost.argtypes = [vp, C.POINTER(cd), vp]
    L.vxba_pgo_optimize.argtypes = [vp, vp, vp, vp, ci, C.POINTER(ci)]
    L.vxba_pgo_stats.argtypes = [vp, _i64p]
    L.vxba_loopreg_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_loopreg_destroy.argtypes = [vp]
    L.vxba_loopreg_last_error.argtypes = [vp]
    L.vxba_loopreg_last_error.restype = C.c_char_p
    L.vxba_loopreg_clear.argtypes = [vp]
    L.vxba_loopreg_num_clouds.argtypes = [vp]
    L.vxba_loopreg_cloud_size.argtypes = [vp, ci]
    L.vxba_loopreg_cloud_size.restype = C.c_int64
    L.vxba_loopreg_read_cloud.argtypes = [vp, ci, vp]
    L.vxba_loopreg_stats.argtypes = [vp, _i64p]
    L.vxba_loopreg_add_cloud.argtypes = [vp, C.c_int64, vp, C.POINTER(ci)]
    L.vxba_loopreg_add_keyframe.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(ci), C.POINTER(C.c_int64)]
    L.vxba_loopreg_associate.argtypes = [vp, ci, ci, _f64p, _f64p, vp, vp]
    L.vxba_loopreg_score.argtypes = [vp, ci, i32p, _f64p, cd, cd, _f64p, _i64p]
    L.vxba_loopreg_icp.argtypes = [vp, ci, i32p, _f64p, vp, _f64p]
    L.vxba_loopsearch_create.argtypes = [ci, vp, C.POINTER(vp)]
    L.vxba_loopsearch_destroy.argtypes = [vp]
    L.vxba_loopsearch_last_error.argtypes = [vp]
    L.vxba_loopsearch_last_error.restype = C.c_char_p
    L.vxba_loopsearch_clear.argtypes = [vp]
    L.vxba_loopsearch_num_frames.argtypes = [vp]
    L.vxba_loopsearch_num_descriptors.argtypes = [vp, ci]
    L.vxba_loopsearch_num_descriptors.restype = C.c_int64
    L.vxba_loopsearch_default_params.argtypes = [vp]
    L.vxba_loopsearch_default_params.restype = None
    L.vxba_loopsearch_describe.argtypes = [vp, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
    L.vxba_loopsearch_read_descriptors.argtypes = [vp, vp, vp, vp]
    L.vxba_loopsearch_search.argtypes = [vp, ci, vp, C.POINTER(ci), C.POINTER(cd), _f64p, C.POINTER(ci), _i64p, _f64p]
    L.vxba_loopsearch_read_matches.argtypes = [vp, C.c_int64, vp, C.POINTER(C.c_int64)]
    L.vxba_loopsearch_add.argtypes = [vp, ci]
    L.vxba_loopsearch_stats.argtypes = [vp, _i64p]
    L.vxba_loopsearch_search_multi.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(ci), ci, vp, C.POINTER(ci), _f64p, _f64p, C.POINTER(ci), _i64p, _f64p]
    L.vxba_loopsearch_read_match_offsets.argtypes = [vp, _i64p]
    f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
    L.vxba_initodom_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_initodom_destroy.argtypes = [vp]
    L.vxba_initodom_last_error.argtypes = [vp]
    L.vxba_initodom_last_error.restype = C.c_char_p
    L.vxba_initodom_clear.argtypes = [vp]
    L.vxba_initodom_cloud_size.argtypes = [vp]
    L.vxba_initodom_cloud_size.restype = C.c_int64
    L.vxba_initodom_cloud.argtypes = [vp, f32p]
    L.vxba_initodom_search.argtypes = [vp, C.c_int64, f32p, i32p, f32p]
    L.vxba_initodom_step.argtypes = [vp, C.c_int64, _f64p, _f64p, _f64p, _f64p, _f64p]
    L.vxba_initodom_inspect.argtypes = [vp, ci, i32p, i32p, _f64p]
    L.vxba_initodom_stats.argtypes = [vp, _i64p]
    L.vxba_init_pose_table.argtypes = [ci, _f64p, _f64p, _f64p, cd, _f64p, _f64p, cd, _f64p]
    L.vxba_init_deskew.argtypes = [ci, C.c_int64, f32p, vp, ci, vp, vp, vp, cd, _f64p, vp, _f64p, cd, ci, C.c_int64, _f64p, i32p, C.POINTER(C.c_int64)]
    L.vxba_init_normal_scatter.argtypes = [vp, _f64p]
    L.vxba_imu_push.argtypes = [_f64p, ci, _f64p, _f64p, _f64p, cd, _f64p, _f64p]
    i64p = np.ctypeslib.ndpointer(dtype=np.int64, flags="C_CONTIGUOUS")
    L.vxba_init_motion_times.argtypes = [_f64p]
    L.vxba_init_motion.argtypes = [vp, vp, ci, i64p, f32p, vp, _f64p, i64p, _f64p, _f64p, _f64p, _f64p, _f64p, _f64p, C.POINTER(InitMotionParams), _f64p, _f64p, _f64p, _f64p,
                                   C.POINTER(ci), _f64p, C.POINTER(ci)]
    L.vxba_keyframe_create.argtypes = [ci, vp, C.POINTER(vp)]
    L.vxba_keyframe_destroy.argtypes = [vp]
    L.vxba_keyframe_last_error.argtypes = [vp]
    L.vxba_keyframe_last_error.restype = C.c_char_p
    L.vxba_keyframe_clear.argtypes = [vp]
    L.vxba_keyframe_push_scan.argtypes = [vp, _f64p, _f64p, C.c_int64, vp, vp, C.POINTER(ci)]
    L.vxba_keyframe_push_scan_device.argtypes = [vp, _f64p, _f64p, C.c_int64, vp, vp, C.POINTER(ci)]
    L.vxba_keyframe_info.argtypes = [vp, C.POINTER(C.c_int64), _f64p, C.POINTER(cd), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.vxba_keyframe_read.argtypes = [vp, vp, vp]
    L.vxba_keyframe_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.vxba_keyframe_device_down_xyz.argtypes = [vp, C.POINTER(vp)]
    L.vxba_keyframe_num_scans.argtypes = [vp]
    L.vxba_keyframe_num_scans.restype = C.c_int64
    L.vxba_keyframe_num_buffered.argtypes = [vp]
    L.vxba_keyframe_scan_poses.argtypes = [vp, C.c_int64, C.c_int64, _f64p, _f64p]
    L.vxba_keyframe_stats.argtypes = [vp, _i64p]
    L.vxba_keyframe_set_profiling.argtypes = [vp, ci]
    L.vxba_keyframe_stage_times.argtypes = [vp, _f64p]
    L.vxba_loopreg_add_keyframe_device.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(ci), C.POINTER(C.c_int64)]
    L.vxba_hba_add_keyframes_device.argtypes = [vp, C.c_int64, vp, vp]
    L.vxba_corner_default_params.argtypes = [vp, ci]
    L.vxba_corner_default_params.restype = None
    L.vxba_corner_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_corner_destroy.argtypes = [vp]
    L.vxba_corner_last_error.argtypes = [vp]
    L.vxba_corner_last_error.restype = C.c_char_p
    L.vxba_corner_extract.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(C.c_int64)]
    L.vxba_corner_extract_device.argtypes = [vp, C.c_int64, vp, vp, C.POINTER(C.c_int64)]
    L.vxba_corner_extract_with_planes.argtypes = [vp, C.c_int64, vp, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
    L.vxba_corner_read.argtypes = [vp, vp, vp, vp]
    L.vxba_corner_planes.argtypes = [vp, C.POINTER(C.c_int64), vp, vp]
    L.vxba_corner_projection_planes.argtypes = [vp, C.POINTER(C.c_int64), vp, vp]
    L.vxba_corner_candidates.argtypes = [vp, C.POINTER(C.c_int64), vp, vp, vp]
    L.vxba_corner_stats.argtypes = [vp, _i64p]
    L.vxba_corner_set_profiling.argtypes = [vp, ci]
    L.vxba_corner_stage_times.argtypes = [vp, _f64p]
    L.vxba_imuekf_default_params.argtypes = [C.POINTER(ImuEkfParams)]
    L.vxba_imuekf_default_params.restype = None
    L.vxba_imuekf_create.argtypes = [ci, C.POINTER(ImuEkfParams), C.POINTER(vp)]
    L.vxba_imuekf_destroy.argtypes = [vp]
    L.vxba_imuekf_last_error.argtypes = [vp]
    L.vxba_imuekf_last_error.restype = C.c_char_p
    L.vxba_imuekf_process.argtypes = [vp, C.c_int64, vp, vp, ci, _f64p, _f64p, _f64p, cd, cd, _f64p, _f64p, _f64p, C.POINTER(ci), _f64p]
    L.vxba_imuekf_read_scan.argtypes = [vp, f32p]
    L.vxba_imuekf_pose_table.argtypes = [vp, _f64p]
    L.vxba_imuekf_reinit.argtypes = [vp, ci, _f64p, _f64p, _f64p, cd, _f64p]
    L.vxba_imuekf_clear.argtypes = [vp]
    L.vxba_imuekf_filter.argtypes = [vp, cd, C.c_int64, C.POINTER(C.c_int64)]
    L.vxba_imuekf_filter_passes.argtypes = [vp]
    L.vxba_imuekf_filtered.argtypes = [vp, f32p]
    L.vxba_imuekf_filtered_device.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    L.vxba_imuekf_stats.argtypes = [vp, _i64p]
    L.vxba_imuekf_set_profiling.argtypes = [vp, ci]
    L.vxba_imuekf_stage_times.argtypes = [vp, _f64p]
    L.vxba_lio_scan_raw_device.argtypes = [vp, C.c_int64, vp, vp, cd, cd]
    L.vxba_intake_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_intake_destroy.argtypes = [vp]
    L.vxba_intake_last_error.argtypes = [vp]
    L.vxba_intake_last_error.restype = C.c_char_p
    L.vxba_intake_push.argtypes = [vp, C.POINTER(ScanLayout), C.c_int64, vp, ci, cd, cd, _f64p]
    L.vxba_intake_push_yaw.argtypes = [vp, C.POINTER(ScanLayout), C.c_int64, vp, ci, cd, cd, _f64p]
    L.vxba_intake_yaw_info.argtypes = [vp, _i64p]
    L.vxba_intake_read.argtypes = [vp, f32p, f32p]
    L.vxba_intake_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.vxba_intake_stats.argtypes = [vp, _i64p]
    L.vxba_intake_set_profiling.argtypes = [vp, ci]
    L.vxba_intake_stage_times.argtypes = [vp, _f64p]
    L.vxba_imuekf_process_device.argtypes = [vp, vp, ci, _f64p, _f64p, _f64p, cd, cd, _f64p, _f64p, _f64p, C.POINTER(ci), _f64p]
    L.vxba_session_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_session_destroy.argtypes = [vp]
    L.vxba_session_last_error.argtypes = [vp]
    L.vxba_session_last_error.restype = C.c_char_p
    L.vxba_session_clear.argtypes = [vp]
    L.vxba_session_load_scans.argtypes = [vp, C.c_int64, _i64p, vp, vp]
    L.vxba_session_num_scans.argtypes = [vp]
    L.vxba_session_num_scans.restype = C.c_int64
    L.vxba_session_build_keyframes.argtypes = [vp, ci, cd, C.POINTER(C.c_int64)]
    L.vxba_session_num_keyframes.argtypes = [vp]
    L.vxba_session_num_keyframes.restype = C.c_int64
    L.vxba_session_keyframes.argtypes = [vp, vp, vp, vp]
    L.vxba_session_read_keyframes.argtypes = [vp, vp]
    L.vxba_session_device.argtypes = [vp, C.POINTER(vp)]
    L.vxba_session_set_scan_poses.argtypes = [vp, vp]
    L.vxba_session_num_windows.argtypes = [C.c_int64, ci, ci]
    L.vxba_session_window_cloud.argtypes = [vp, ci, ci, ci, C.POINTER(C.c_int64), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.vxba_session_read_window.argtypes = [vp, vp]
    L.vxba_session_stats.argtypes = [vp, _i64p]
    L.vxba_session_set_profiling.argtypes = [vp, ci]
    L.vxba_session_stage_times.argtypes = [vp, _f64p]
    L.vxba_globalmap.argtypes = [ci, ci, C.POINTER(vp), C.POINTER(vp), _i64p, C.POINTER(vp), f32p, C.c_int64, vp, C.c_int64, C.POINTER(C.c_int64), vp, C.POINTER(C.c_int64)]
    L.vxba_hba_device_clouds.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.vxba_map_loop_update_device.argtypes = [vp, ci, vp, vp, vp, cd, ci, vp, vp]
    L.vxba_map_scan_device.argtypes = [vp, ci, C.POINTER(C.c_int64), C.POINTER(vp), C.POINTER(vp)]
    L.vxba_kfarchive_create.argtypes = [ci, C.POINTER(vp)]
    L.vxba_kfarchive_destroy.argtypes = [vp]
    L.vxba_kfarchive_last_error.argtypes = [vp]
    L.vxba_kfarchive_last_error.restype = C.c_char_p
    L.vxba_kfarchive_clear.argtypes = [vp]
    L.vxba_kfarchive_add.argtypes = [vp, C.c_int64, _f64p, cd, C.c_int64, vp]
    L.vxba_kfarchive_add_device.argtypes = [vp, C.c_int64, _f64p, cd, C.c_int64, vp]
    L.vxba_kfarchive_num.argtypes = [vp]
    L.vxba_kfarchive_num.restype = C.c_int64
    L.vxba_kfarchive_info.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64), _f64p, C.POINTER(cd), C.POINTER(C.c_int64), C.POINTER(ci)]
    L.vxba_kfarchive_read.argtypes = [vp, C.c_int64, vp]
    L.vxba_kfarchive_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.vxba_kfarchive_set_poses.argtypes = [vp, vp]
    L.vxba_kfarchive_arm_history.argtypes = [vp, ci]
    L.vxba_kfarchive_history_size.argtypes = [vp]
    L.vxba_kfarchive_history_size.restype = C.c_int64
    L.vxba_kfarchive_load_near.argtypes = [vp, _f64p, cd, C.POINTER(ci), C.POINTER(C.c_int64), C.POINTER(vp)]
    L.vxba_kfarchive_map_loop.argtypes = [vp, ci, ci, _i64p, C.POINTER(ci), C.POINTER(vp), C.POINTER(vp)]
    L.vxba_kfarchive_map_loop_scans.argtypes = [vp, ci, ci, ci, vp, vp, vp, vp, _i64p, C.POINTER(ci), C.POINTER(vp), C.POINTER(vp)]
    L.vxba_kfarchive_stats.argtypes = [vp, _i64p]
    _lib = L
    return L


def _c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _opt(a):
    """Optional f64 array -> pointer (or NULL); returns (pointer, keepalive)."""
    if a is None:
        return None, None
    arr = _c(a)
    return arr.ctypes.data_as(C.c_void_p), arr


def _ptr(a):
    """ndarray or None -> ``c_void_p`` (NULL for None); the pointer object holds a reference to the array, which so outlives the call."""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(addr):
    """Raw device address (an int, e.g. a tensor's ``data_ptr()``; 0 or None: none) -> ``c_void_p``."""
    return C.c_void_p(int(addr) if addr else None)


class _Handle:
    """One object of the C ABI's ``<_prefix>_create`` / ``_destroy`` / ``_last_error`` families and what every owner of one does the same way:
    create (``VxbaError`` on failure, there is no CPU fallback), the error check, an idempotent ``close``, a guarded finaliser and ``with``.
    ``_h`` is a non-null ``c_void_p`` while the handle is open and an empty (false) one otherwise -- before create, after a failed one, after close.
    ``LidarFactor`` and ``HbaSession`` still carry their own copies of this."""
    _prefix = None
    _h = C.c_void_p()

    def _create(self, *args):
        """``<_prefix>_create(*args, &handle)``."""
        self._L = load_library()
        h = C.c_void_p()
        rc = getattr(self._L, self._prefix + "_create")(*args, C.byref(h))
        if rc != 0:
            raise VxbaError(f"{self._prefix}_create failed: {_ERRNAMES.get(rc, rc)} (needs a gfx950 GPU; there is no CPU fallback)")
        self._h = h

    def _check(self, rc, what=None):
        """A non-zero return code -> ``VxbaError("[<what>: ]<VXBA_ERR_*>: <the handle's last_error text>")``."""
        if rc != 0:
            msg = getattr(self._L, self._prefix + "_last_error")(self._h)
            raise VxbaError(f"{what + ': ' if what else ''}{_ERRNAMES.get(rc, rc)}: {msg.decode() if msg else ''}")

    _chk = _check

    def close(self):
        if self._h:
            getattr(self._L, self._prefix + "_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001 - a finaliser has nobody to raise to (interpreter shutdown, a half-built object)
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class LidarFactor:
    """The LiDAR BA factor on one MI355X (reference: voxel_map.hpp:109-290)."""

    def __init__(self, win_size: int, device: int = 0):
        self._L = load_library()
        self._h = C.c_void_p()
        rc = self._L.vxba_create(int(win_size), int(device), C.byref(self._h))
        if rc != 0:
            self._h = C.c_void_p()
            raise VxbaError(f"vxba_create(win_size={win_size}, device={device}) failed: {_ERRNAMES.get(rc, rc)} "
                            "(needs a gfx950 GPU; there is no CPU fallback)")
        self._cb = None
        self._owned = True

    @classmethod
    def from_handle(cls, handle):
        """A view of a factor somebody else owns (the top-level factor of an ``HbaSession``): every method works, ``close`` leaves it alone."""
        self = cls.__new__(cls)
        self._L = load_library()
        self._h = C.c_void_p(handle if isinstance(handle, int) else handle.value)
        self._cb = None
        self._owned = False
        return self

    # -- plumbing -------------------------------------------------------------------------------
    def _chk(self, rc):
        if rc != 0:
            msg = self._L.vxba_last_error(self._h)
            raise VxbaError(f"{_ERRNAMES.get(rc, rc)}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            if getattr(self, "_owned", True):
                self._L.vxba_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    @property
    def win_size(self) -> int:
        return self._L.vxba_win_size(self._h)

    @win_size.setter
    def win_size(self, w: int):
        self._chk(self._L.vxba_set_win_size(self._h, int(w)))

    def size(self) -> int:
        """``plvec_voxels.size()``"""
        return self._L.vxba_size(self._h)

    def __len__(self):
        return self.size()

    def set_stream(self, hip_stream: int | None):
        self._chk(self._L.vxba_set_stream(self._h, C.c_void_p(hip_stream or 0)))

    def reserve(self, n):
        self._chk(self._L.vxba_reserve(self._h, int(n)))

    # -- construction ---------------------------------------------------------------------------
    def push_voxel(self, vec_orig, fix, coe, eig_value, eig_vector, pcr_add):
        """Single-voxel form of voxel_map.hpp:122-130 (all arguments in packed format)."""
        self.push_voxels(np.asarray(vec_orig)[None], np.asarray(fix)[None], [coe], np.asarray(eig_value)[None],
                         np.asarray(eig_vector).reshape(1, 9), np.asarray(pcr_add)[None])

    def push_voxels(self, clusters, fix, coe, eig_val=None, eig_vec=None, merged=None):
        clusters = _c(clusters)
        n = clusters.shape[0]
        if clusters.shape != (n, self.win_size, 10):
            raise VxbaError(f"clusters must be (n, {self.win_size}, 10)")
        pv, kv = _opt(eig_val)
        pu, ku = _opt(eig_vec)
        pm, km = _opt(merged)
        self._chk(self._L.vxba_push_voxels(self._h, n, clusters, _c(fix), _c(coe), pv, pu, pm))

    def push_voxels_csr(self, row_ptr, frame_idx, clusters, fix, coe, eig_val=None, eig_vec=None, merged=None):
        """push_voxels for sparse incidence: voxel a's observed frames are frame_idx[row_ptr[a]:row_ptr[a + 1]] (strictly increasing), their
        clusters the matching rows of ``clusters`` (nnz, 10).  Nothing dense is built on the host or sent over PCIe."""
        rp = np.ascontiguousarray(row_ptr, dtype=np.int64)
        fr = np.ascontiguousarray(frame_idx, dtype=np.int32)
        cl = _c(clusters).reshape(-1, 10)
        n = rp.size - 1
        if n < 0 or cl.shape[0] != fr.size or (n >= 0 and rp.size and rp[-1] != fr.size):
            raise VxbaError("push_voxels_csr: row_ptr[-1], frame_idx and clusters disagree on the number of entries")
        pv, kv = _opt(eig_val)
        pu, ku = _opt(eig_vec)
        pm, km = _opt(merged)
        self._chk(self._L.vxba_push_voxels_csr(self._h, n, rp.ctypes.data_as(C.c_void_p), fr.ctypes.data_as(C.c_void_p), cl.ctypes.data_as(C.c_void_p), _c(fix), _c(coe), pv, pu, pm))

    def push_points(self, n_voxels, xyz_body, cell_ptr, fix=None, coe=None):
        """K1: build the clusters of ``n_voxels`` voxels on the GPU from bucketed body-frame points."""
        xyz = _c(xyz_body).reshape(-1, 3)
        ptr = np.ascontiguousarray(cell_ptr, dtype=np.int64)
        pf, kf = _opt(fix)
        pc, kc = _opt(coe)
        self._chk(self._L.vxba_push_points(self._h, int(n_voxels), xyz.shape[0], xyz, ptr, pf, pc))

    def voxelize_push(self, xyz_local, frame_ptr, xs, params: "VoxelizeParams", want_ids=True):
        """OctreeGBA::cut_voxel + recut on the GPU (loop_refine.hpp:273-476): appends the factor voxels found in the window's
        points; returns their canonical node ids (uint64) in push order (or just the count)."""
        xyz = _c(xyz_local).reshape(-1, 3)
        fp = np.ascontiguousarray(frame_ptr, dtype=np.int64)
        n = C.c_int64(0)
        cap = self._ids_cap(xyz.shape[0], params) if want_ids else 0
        ids = np.zeros(max(cap, 1), dtype=np.uint64)
        self._chk(self._L.vxba_voxelize_push(self._h, xyz.shape[0], xyz, fp, _c(xs), C.byref(params), C.byref(n),
                                             ids.ctypes.data_as(C.c_void_p) if want_ids else None, cap))
        return ids[: n.value].copy() if want_ids else n.value

    @staticmethod
    def _ids_cap(n_points, params):
        floor_pts = min([params.min_points] + [v for v in params.min_points_layer[: params.max_layer + 1] if v > 0])
        return n_points // (max(floor_pts, 0) + 1) + 1

    def voxelize_push_device(self, d_xyz_ptr: int, n_points: int, frame_ptr, xs, params: "VoxelizeParams", want_ids=True):
        """:meth:`voxelize_push` on points that already live in device memory (``d_xyz_ptr``: n_points x 3 float64, e.g. a torch
        tensor's ``data_ptr()``)."""
        fp = np.ascontiguousarray(frame_ptr, dtype=np.int64)
        n = C.c_int64(0)
        cap = self._ids_cap(n_points, params) if want_ids else 0
        ids = np.zeros(max(cap, 1), dtype=np.uint64)
        self._chk(self._L.vxba_voxelize_push_device(self._h, int(n_points), C.c_void_p(d_xyz_ptr), fp, _c(xs), C.byref(params), C.byref(n),
                                                    ids.ctypes.data_as(C.c_void_p) if want_ids else None, cap))
        return ids[: n.value].copy() if want_ids else n.value

    def read_clusters(self, head=0, end=None):
        end = self.size() if end is None else end
        out = np.zeros((end - head, self.win_size, 10))
        self._chk(self._L.vxba_read_clusters(self._h, head, end, out))
        return out

    def clear(self):
        self._chk(self._L.vxba_clear(self._h))

    # -- sweeps ---------------------------------------------------------------------------------
    def acc_evaluate2(self, xs, head=0, end=None):
        """Returns (Hess[r, c], JacT, residual) for voxels [head, end) under packed poses ``xs`` (W, 12)."""
        end = self.size() if end is None else end
        n = 6 * self.win_size
        H = np.zeros((n, n)); J = np.zeros(n); r = C.c_double(0)
        self._chk(self._L.vxba_acc_evaluate2(self._h, _c(xs), head, end, H, J, C.byref(r)))
        return H.T.copy(), J, r.value   # column-major on the wire

    def evaluate_only_residual(self, xs, head=0, end=None):
        end = self.size() if end is None else end
        r = C.c_double(0)
        self._chk(self._L.vxba_evaluate_only_residual(self._h, _c(xs), head, end, C.byref(r)))
        return r.value

    def packed_len(self) -> int:
        return self._L.vxba_packed_len(self._h)

    def acc_evaluate2_device(self, xs, d_out_ptr: int, head=0, end=None):
        end = self.size() if end is None else end
        self._chk(self._L.vxba_acc_evaluate2_device(self._h, _c(xs), head, end, C.c_void_p(d_out_ptr)))

    def evaluate_only_residual_device(self, xs, d_out_ptr: int, head=0, end=None):
        end = self.size() if end is None else end
        self._chk(self._L.vxba_evaluate_only_residual_device(self._h, _c(xs), head, end, C.c_void_p(d_out_ptr)))

    def read_cache(self, head=0, end=None):
        """(eig_values (n,3), eig_vectors (n,9 col-major), pcr_adds (n,10)) of voxels [head, end)."""
        end = self.size() if end is None else end
        n = end - head
        ev = np.zeros((n, 3)); U = np.zeros((n, 9)); m = np.zeros((n, 10))
        self._chk(self._L.vxba_read_cache(self._h, head, end, ev, U, m))
        return ev, U, m

    def snapshot_cache(self):
        self._chk(self._L.vxba_snapshot_cache(self._h))

    def restore_cache(self):
        self._chk(self._L.vxba_restore_cache(self._h))

    # -- multi-GPU hook -------------------------------------------------------------------------
    def set_allreduce(self, fn):
        """``fn(device_ptr: int, count: int, hip_stream: int) -> None`` sums f64 across voxel shards in place."""
        if fn is None:
            self._cb = None
            self._chk(self._L.vxba_set_allreduce(self._h, C.cast(None, _ALLREDUCE_FN), None))
            return

        def tramp(ctx, ptr, count, stream):
            try:
                fn(int(ptr or 0), int(count), int(stream or 0))
                return 0
            except Exception:  # noqa: BLE001 - must not unwind through C
                import traceback
                traceback.print_exc()
                return 1

        self._cb = _ALLREDUCE_FN(tramp)
        self._chk(self._L.vxba_set_allreduce(self._h, self._cb, None))

    def rccl_attach(self, librccl_path: str, nranks: int, rank: int, unique_id: bytes):
        """Direct RCCL all-reduce of the exchange buffers inside the device-resident LM loop (collective call)."""
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._chk(self._L.vxba_rccl_attach(self._h, librccl_path.encode(), int(nranks), int(rank), C.cast(buf, C.c_void_p)))

    def rccl_detach(self):
        self._chk(self._L.vxba_rccl_detach(self._h))

    def use_external_buffers(self, d_packed_ptr: int | None, d_scalar_ptr: int | None):
        self._chk(self._L.vxba_use_external_buffers(self._h, C.c_void_p(d_packed_ptr or 0), C.c_void_p(d_scalar_ptr or 0)))

    # -- measurement ----------------------------------------------------------------------------
    def peer_export(self) -> bytes:
        """64-byte IPC handle of this factor's all-reduce mailbox (vxba_peer_export)."""
        buf = C.create_string_buffer(64)
        self._chk(self._L.vxba_peer_export(self._h, buf))
        return buf.raw

    def peer_attach(self, nranks: int, rank: int, handles):
        """handles: the ranks' peer_export() results in rank order."""
        blob = b"".join(handles)
        assert len(blob) == 64 * nranks
        self._chk(self._L.vxba_peer_attach(self._h, int(nranks), int(rank), C.c_char_p(blob)))

    def peer_detach(self):
        self._chk(self._L.vxba_peer_detach(self._h))

    def peer_selftest(self) -> bool:
        ok = C.c_int(0)
        self._chk(self._L.vxba_peer_selftest(self._h, C.byref(ok)))
        return bool(ok.value)

    def peer_status(self) -> int:
        st = C.c_int(0)
        self._chk(self._L.vxba_peer_status(self._h, C.byref(st)))
        return st.value

    OPTIONS = {"fused_solve": 0, "spec_collective": 1, "wide_device_solve": 2, "k2_voxels_per_block": 4,
               "debug_solve_timeout": 5, "li_structured_solve": 6, "li_queued_sweeps": 7, "li_device_pose_solve": 8, "fused_sweeps": 9, "stat_fused_fallbacks": 100, "stat_li_last_call_us": 101, "stat_li_device_fallbacks": 102, "stat_reject_heavy": 103}

    def set_option(self, name: str, value: int):
        """Execution options of include/vxba.h (VXBA_OPT_*): fused_solve, spec_collective, wide_device_solve, k2_voxels_per_block."""
        self._chk(self._L.vxba_set_option(self._h, self.OPTIONS[name], int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        self._chk(self._L.vxba_get_option(self._h, self.OPTIONS[name], C.byref(v)))
        return v.value

    def set_precision(self, mode: str):
        """'f64' (default), 'mixed' (f32 products on the matrix cores, f64 accumulation; BASELINE configs[2]) or 'mixed_f32_clusters'
        (mixed, and the residual sweep reads f32 re-centred cluster records)."""
        self._chk(self._L.vxba_set_precision(self._h, {"f64": 0, "mixed": 1, "mixed_f32_clusters": 2}[mode]))

    def set_profiling(self, mask: int):
        """Bit mask of kernels to time with events: 1 K3, 2 K2, 4 K3 finalize, 8 K1, 16 all-reduce, 32 the fused launch (0 = off)."""
        self._chk(self._L.vxba_set_profiling(self._h, int(mask)))

    def kernel_times(self, reset=False):
        ms = np.zeros(4); calls = np.zeros(4, dtype=np.int64)
        self._chk(self._L.vxba_get_kernel_times(self._h, ms, calls, int(reset)))
        names = ("k3_hessian", "k2_residual", "k3_finalize", "k1_build")
        return {k: dict(ms_sum=float(ms[i]), calls=int(calls[i])) for i, k in enumerate(names)}

    def collective_time(self, reset=False):
        """All-reduces of a voxel-sharded factor bracketed while profiling bit 16 was set: dict(ms_sum, calls)."""
        ms = C.c_double(0); calls = C.c_int64(0)
        self._chk(self._L.vxba_get_collective_time(self._h, C.byref(ms), C.byref(calls), int(reset)))
        return dict(ms_sum=float(ms.value), calls=int(calls.value))

    def fused_time(self, reset=False):
        """Fused solve + residual + Hessian launches bracketed while profiling bit 32 was set: dict(ms_sum, calls)."""
        ms = C.c_double(0); calls = C.c_int64(0)
        self._chk(self._L.vxba_get_fused_time(self._h, C.byref(ms), C.byref(calls), int(reset)))
        return dict(ms_sum=float(ms.value), calls=int(calls.value))

    def algorithmic_bytes(self):
        b = np.zeros(2)
        self._chk(self._L.vxba_algorithmic_bytes(self._h, b))
        return dict(k3=float(b[0]), k2=float(b[1]))

    def nnz(self) -> int:
        v = C.c_int64(0)
        self._chk(self._L.vxba_nnz(self._h, C.byref(v)))
        return v.value

    def device_bytes(self):
        """Device memory held by the factor: dict(store, work, scratch, total) in bytes (vxba_device_bytes)."""
        b = (C.c_int64 * 4)()
        self._chk(self._L.vxba_device_bytes(self._h, b))
        return dict(store=int(b[0]), work=int(b[1]), scratch=int(b[2]), total=int(b[3]))

    def lm_steps(self, xs_init, n_steps, steps_per_solve=3):
        """Bench driver: returns (poses, [residual1, residual2] of the last step, dict(iters, accepted, rejected))."""
        out = np.zeros((self.win_size, 12)); resis = np.zeros(2); st = np.zeros(3, dtype=np.int64)
        self._chk(self._L.vxba_lm_steps(self._h, _c(xs_init), int(n_steps), int(steps_per_solve), out, resis, st))
        return out, resis, dict(iters=int(st[0]), accepted=int(st[1]), rejected=int(st[2]))


class Lidar_BA_Optimizer:
    """The LM shell that owns the loop (reference: voxel_map.hpp:293-444)."""

    def damping_iter(self, x_stats, voxhess: LidarFactor, max_iter: int = 3):
        """Returns dict(poses, hess, resis, trace, is_converge); ``x_stats`` (W,12) is not modified."""
        W = voxhess.win_size
        n = 6 * W
        Rp = _c(x_stats).copy()
        hess = np.zeros((n, n)); resis = np.zeros(2); trace = np.zeros((max(max_iter, 1), TRACE_COLS))
        nt = C.c_int(0); conv = C.c_int(0)
        voxhess._chk(voxhess._L.vxba_damping_iter(voxhess.handle, Rp, int(max_iter), hess, resis, trace, C.byref(nt), C.byref(conv)))
        return dict(poses=Rp, hess=hess.T.copy(), resis=resis, trace=trace[: nt.value].copy(), is_converge=bool(conv.value))


STATE_LEN, IMU_LEN, LI_DIM = 24, 304, 15


def pack_state(R, p, v=None, bg=None, ba=None, g=None):
    """One window state in the flat C-ABI format [R col-major | p | v | bg | ba | g] (tools.hpp:135-199)."""
    z = np.zeros(3)
    return np.concatenate([np.asarray(R, dtype=np.float64).T.reshape(9), p, z if v is None else v, z if bg is None else bg,
                           z if ba is None else ba, z if g is None else g]).astype(np.float64)


class IMU_PRE:
    """Preintegrated IMU factor between two consecutive frames (reference: preintegration.hpp:11-310), host-side.
    ``blob`` is the flat VXBA_IMU_LEN record; fields are views into it."""

    _FIELDS = dict(R_delta=(0, 9), p_delta=(9, 3), v_delta=(12, 3), bg=(15, 3), ba=(18, 3), R_bg=(21, 9), p_bg=(30, 9), p_ba=(39, 9),
                   v_bg=(48, 9), v_ba=(57, 9), dtime=(66, 1), dbg=(67, 3), dba=(70, 3), dbg_buf=(73, 3), dba_buf=(76, 3), cov=(79, 225))

    def __init__(self, bg=None, ba=None, blob=None):
        self._L = load_library()
        if blob is not None:
            self.blob = _c(blob).copy()
            assert self.blob.shape == (IMU_LEN,)
        else:
            self.blob = np.zeros(IMU_LEN)
            pb, kb = _opt(bg); pa, ka = _opt(ba)
            rc = self._L.vxba_imu_init(self.blob, pb, pa)
            if rc:
                raise VxbaError(f"vxba_imu_init failed ({rc})")

    def field(self, name):
        o, n = self._FIELDS[name]
        a = self.blob[o:o + n]
        if n == 9:
            return a.reshape(3, 3).T
        if n == 225:
            return a.reshape(15, 15).T
        return a[0] if n == 1 else a

    def push_imu(self, stamps, gyr, acc, scale, noise_meas, noise_walk):
        """``push_imu`` (preintegration.hpp:50-73) on raw messages: stamps K, gyr / acc K x 3; mid-point samples, acc * scale, minus the factor's biases."""
        st = _c(stamps).reshape(-1)
        rc = self._L.vxba_imu_push(self.blob, st.shape[0], st, _c(gyr).reshape(-1, 3), _c(acc).reshape(-1, 3), float(scale),
                                   np.ascontiguousarray(np.asarray(noise_meas, dtype=np.float64).T), np.ascontiguousarray(np.asarray(noise_walk, dtype=np.float64).T))
        if rc:
            raise VxbaError(f"vxba_imu_push failed ({rc})")

    def add_imu(self, cur_gyr, cur_acc, dt, noise_meas, noise_walk):
        """One bias-corrected mid-point sample (preintegration.hpp:75-135); noise_* are the 6x6 noiseMeas / noiseWalk."""
        rc = self._L.vxba_imu_add(self.blob, _c(cur_gyr), _c(cur_acc), float(dt), _c(np.asarray(noise_meas).T), _c(np.asarray(noise_walk).T))
        if rc:
            raise VxbaError(f"vxba_imu_add failed ({rc})")

    def give_evaluate(self, st1, st2, jac_enable=True):
        """Returns (residual, jtj (30,30), gg (30,)) -- jtj/gg are None without jac_enable (preintegration.hpp:137-212)."""
        r = C.c_double(0)
        if jac_enable:
            jtj = np.zeros((30, 30)); gg = np.zeros(30)
            rc = self._L.vxba_imu_evaluate(self.blob, _c(st1), _c(st2), 1, _ptr(jtj), _ptr(gg), C.byref(r))
            if rc:
                raise VxbaError(f"vxba_imu_evaluate failed ({_ERRNAMES.get(rc, rc)})")
            return r.value, jtj.T.copy(), gg
        rc = self._L.vxba_imu_evaluate(self.blob, _c(st1), _c(st2), 0, None, None, C.byref(r))
        if rc:
            raise VxbaError(f"vxba_imu_evaluate failed ({_ERRNAMES.get(rc, rc)})")
        return r.value, None, None

    def give_evaluate_g(self, st1, st2):
        """give_evaluate with the gravity columns (preintegration.hpp:214-294): (residual, jtj (33,33), gg (33,))."""
        r = C.c_double(0)
        jtj = np.zeros((33, 33)); gg = np.zeros(33)
        rc = self._L.vxba_imu_evaluate_g(self.blob, _c(st1), _c(st2), 1, _ptr(jtj), _ptr(gg), C.byref(r))
        if rc:
            raise VxbaError(f"vxba_imu_evaluate_g failed ({_ERRNAMES.get(rc, rc)})")
        return r.value, jtj.T.copy(), gg

    def update_state(self, dxi15):
        self._L.vxba_imu_update_state(self.blob, _c(dxi15))


def hess_plus(win_size, Hess15, JacT15, Hess6, JacT6):
    """LI_BA_Optimizer::hess_plus (voxel_map.hpp:455-463) on (r, c)-indexed numpy arrays; returns the updated copies."""
    H = _c(np.asarray(Hess15).T).copy(); J = _c(JacT15).copy()
    rc = load_library().vxba_hess_plus(int(win_size), H, J, _c(np.asarray(Hess6).T), _c(JacT6))
    if rc:
        raise VxbaError(f"vxba_hess_plus failed ({rc})")
    return H.T.copy(), J


class LI_BA_Optimizer:
    """The LiDAR-inertial LM shell (reference: voxel_map.hpp:446-655): 15 unknowns per frame, IMU factors between
    consecutive frames, voxel sweeps on the GPU."""

    def __init__(self, imu_coef: float = 1e-4):
        self.imu_coef = float(imu_coef)

    @staticmethod
    def _blobs(imus_factor):
        return _c(np.stack([f.blob for f in imus_factor])) if len(imus_factor) else np.zeros((0, IMU_LEN))

    def divide_thread(self, x_stats, voxhess: LidarFactor, imus_factor):
        """Returns (Hess (15W,15W), JacT (15W,), residual)."""
        n = LI_DIM * voxhess.win_size
        H = np.zeros((n, n)); J = np.zeros(n); r = C.c_double(0)
        voxhess._chk(voxhess._L.vxba_li_evaluate(voxhess.handle, _c(x_stats), self._blobs(imus_factor), self.imu_coef, H, J, C.byref(r)))
        return H.T.copy(), J, r.value

    def only_residual(self, x_stats, voxhess: LidarFactor, imus_factor):
        r = C.c_double(0)
        voxhess._chk(voxhess._L.vxba_li_only_residual(voxhess.handle, _c(x_stats), self._blobs(imus_factor), self.imu_coef, C.byref(r)))
        return r.value

    def damping_iter(self, x_stats, voxhess: LidarFactor, imus_factor, max_iter: int = 3):
        """Returns dict(states, hess, trace); the IMU factors' dbg/dba are updated in place like upstream (:608-609)."""
        W = voxhess.win_size
        n = LI_DIM * W
        st = _c(x_stats).copy()
        blobs = self._blobs(imus_factor)
        hess = np.empty((n, n)) if max_iter > 0 else np.zeros((n, n))   # written in full by the library when an iteration runs
        trace = np.zeros((max(max_iter, 1), TRACE_COLS)); nt = C.c_int(0)
        voxhess._chk(voxhess._L.vxba_li_damping_iter(voxhess.handle, st, blobs, self.imu_coef, int(max_iter), _ptr(hess),
                                                     _ptr(trace), C.byref(nt)))
        for f, b in zip(imus_factor, blobs):
            f.blob[:] = b
        return dict(states=st, hess=hess.T, trace=trace[: nt.value])   # hess: (r, c)-indexed view of the column-major output, no copy


class LI_BA_OptimizerGravity(LI_BA_Optimizer):
    """LI_BA_Optimizer with the gravity vector as three more unknowns (reference: voxel_map.hpp:658-864)."""

    def divide_thread(self, x_stats, voxhess: LidarFactor, imus_factor):
        """The (15W+3)-dimensional joint system (voxel_map.hpp:673-736): returns (Hess[r, c], JacT, residual)."""
        W = voxhess.win_size
        n = LI_DIM * W + 3
        Hess = np.zeros((n, n)); JacT = np.zeros(n); r = C.c_double(0)
        voxhess._chk(voxhess._L.vxba_li_evaluate_gravity(voxhess.handle, _c(x_stats), self._blobs(imus_factor), self.imu_coef, Hess, JacT, C.byref(r)))
        return Hess.T.copy(), JacT, r.value

    # only_residual: inherited -- give_evaluate_g without Jacobian is give_evaluate without Jacobian (voxel_map.hpp:738-773)

    def damping_iter(self, x_stats, voxhess: LidarFactor, imus_factor, max_iter: int = 2):
        W = voxhess.win_size
        n = LI_DIM * W + 3
        st = _c(x_stats).copy()
        blobs = self._blobs(imus_factor)
        hess = np.empty((n, n)) if max_iter > 0 else np.zeros((n, n))
        resis = np.zeros(2); trace = np.zeros((max(max_iter, 1), TRACE_COLS)); nt = C.c_int(0)
        voxhess._chk(voxhess._L.vxba_li_damping_iter_gravity(voxhess.handle, st, blobs, self.imu_coef, int(max_iter), _ptr(hess),
                                                             resis, _ptr(trace), C.byref(nt)))
        for f, b in zip(imus_factor, blobs):
            f.blob[:] = b
        return dict(states=st, hess=hess.T, resis=resis, trace=trace[: nt.value])


def damping_iter_generic(win_size: int, x_stats, hess_fn, resid_fn, max_iter: int = 3):
    """``Lidar_BA_Optimizer::damping_iter`` over caller-supplied sweeps (host-only; no GPU needed).

    ``hess_fn(xs (W,12)) -> (Hess[r,c] (n,n), JacT (n,), residual)`` and ``resid_fn(xs) -> residual`` -- typically a local
    voxel shard's sweep followed by an all-reduce (see :mod:`voxel_slam_amd.dist`)."""
    L = load_library()
    W = int(win_size); n = 6 * W
    Rp = _c(x_stats).copy()

    def _h(ctx, rp, packed):
        try:
            xs = np.ctypeslib.as_array(rp, shape=(W, 12)).copy()
            H, J, r = hess_fn(xs)
            out = np.ctypeslib.as_array(packed, shape=(n * n + n + 1,))
            out[: n * n] = np.asarray(H, dtype=np.float64).T.reshape(-1)   # column-major on the wire
            out[n * n: n * n + n] = J
            out[n * n + n] = r
            return 0
        except Exception:  # noqa: BLE001 - must not unwind through C
            import traceback
            traceback.print_exc()
            return 1

    def _r(ctx, rp, res):
        try:
            res[0] = float(resid_fn(np.ctypeslib.as_array(rp, shape=(W, 12)).copy()))
            return 0
        except Exception:  # noqa: BLE001
            import traceback
            traceback.print_exc()
            return 1

    hess = np.zeros((n, n)); resis = np.zeros(2); trace = np.zeros((max(max_iter, 1), TRACE_COLS))
    nt = C.c_int(0); conv = C.c_int(0)
    rc = L.vxba_damping_iter_generic(W, Rp, int(max_iter), _HESS_FN(_h), _RESID_FN(_r), None, hess, resis, trace, C.byref(nt), C.byref(conv))
    if rc != 0:
        raise VxbaError(f"vxba_damping_iter_generic failed: {_ERRNAMES.get(rc, rc)}")
    return dict(poses=Rp, hess=hess.T.copy(), resis=resis, trace=trace[: nt.value].copy(), is_converge=bool(conv.value))


LIO_SWEEP_LEN = 52
LIO_MAX_ITER = 4


def unpack_sweep(sw):
    """One sweep record -> dict(HTH 6x6, HTz 6, nnt 3x3, match_num)."""
    sw = np.asarray(sw)
    return {"HTH": sw[:36].reshape(6, 6).T.copy(), "HTz": sw[36:42].copy(), "nnt": sw[42:51].reshape(3, 3).T.copy(), "match_num": int(sw[51])}


class LioEstimator(_Handle):
    """The odometry's point-to-plane update on the GPU: the plane map (``surf_map`` flattened to its leaves), the current scan
    (``pptr``) and ``lio_state_estimation`` (voxelslam.cpp:855-958) with ``match`` (voxel_map.hpp:1335-1392, 1674-1698).
    States are the flat VXBA state vectors of :func:`pack_state`, covariances 15x15 (tangent order [dphi dp dv dbg dba])."""
    _prefix = "vxba_lio"

    def __init__(self, voxel_size: float = 1.0, max_layer: int = 2, device: int = 0):
        self._create(float(voxel_size), int(max_layer), int(device))
        self.voxel_size, self.max_layer = float(voxel_size), int(max_layer)

    def set_option(self, name: str, value: int):
        """VXBA_LIO_OPT_*: 'device_ekf' (1 = EKF update as a kernel, default; 0 = host algebra between sweeps)."""
        self._chk(self._L.vxba_lio_set_option(self._h, {"device_ekf": 0}[name], int(value)))

    # -- map ------------------------------------------------------------------------------------------------------------
    def map_update(self, loc, layer, path, center, normal, plane_var, radius, is_plane=None):
        """Upsert leaves.  plane_var: n x 6 x 6 (numpy order; symmetric up to round-off, sent column-major)."""
        loc = np.ascontiguousarray(loc, dtype=np.int64).reshape(-1, 3)
        n = loc.shape[0]
        layer = np.ascontiguousarray(layer, dtype=np.int32); path = np.ascontiguousarray(path, dtype=np.int32)
        pv = np.ascontiguousarray(np.transpose(np.asarray(plane_var, dtype=np.float64).reshape(n, 6, 6), (0, 2, 1)))
        isp = None if is_plane is None else np.ascontiguousarray(is_plane, dtype=np.int32)
        self._chk(self._L.vxba_lio_map_update(self._h, n, loc, layer, path, _ptr(isp), _c(center), _c(normal), pv, _c(radius)))

    def map_clear(self):
        self._chk(self._L.vxba_lio_map_clear(self._h))

    def map_size(self):
        a, b = C.c_int64(), C.c_int64()
        self._chk(self._L.vxba_lio_map_size(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- scan -----------------------------------------------------------------------------------------------------------
    def var_init(self, xyz, ext_R=None, ext_p=None, dept_err=0.02, beam_err=0.05):
        """``var_init`` (voxelslam.hpp:187-201) on sensor-frame float32 points."""
        xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        ext = None
        if ext_R is not None:
            ext = np.concatenate([np.asarray(ext_R, dtype=np.float64).T.reshape(9), np.zeros(3) if ext_p is None else np.asarray(ext_p, dtype=np.float64)])
        self._chk(self._L.vxba_lio_scan_raw(self._h, xyz.shape[0], xyz, _ptr(ext), float(dept_err), float(beam_err)))

    def var_init_device(self, d_xyz, n, ext=None, dept_err=0.02, beam_err=0.05):
        """``var_init`` on a float32 cloud that lies in device memory (:meth:`ImuEkf.filtered_device`); ext = [R 9 column-major | p 3] or None."""
        e = None if ext is None else _c(ext).reshape(12)
        self._chk(self._L.vxba_lio_scan_raw_device(self._h, int(n), d_xyz, _ptr(e), float(dept_err), float(beam_err)))

    def set_points(self, pnt, var):
        """Ready ``pointVar`` arrays: pnt n x 3, var n x 3 x 3."""
        pnt = _c(pnt).reshape(-1, 3)
        var = np.ascontiguousarray(np.transpose(np.asarray(var, dtype=np.float64).reshape(-1, 3, 3), (0, 2, 1)))
        self._chk(self._L.vxba_lio_scan_set(self._h, pnt.shape[0], pnt, var))

    def scan_size(self) -> int:
        return int(self._L.vxba_lio_scan_size(self._h))

    def read_points(self):
        n = self.scan_size()
        pnt = np.zeros((n, 3)); var = np.zeros((n, 9))
        self._chk(self._L.vxba_lio_scan_read(self._h, pnt, var))
        return pnt, np.transpose(var.reshape(n, 3, 3), (0, 2, 1)).copy()

    # -- the path -------------------------------------------------------------------------------------------------------
    @staticmethod
    def _cov(cov):
        return np.ascontiguousarray(np.asarray(cov, dtype=np.float64).reshape(15, 15).T)

    def sweep(self, state, cov, reset_cache=True, want_points=False):
        out = np.zeros(LIO_SWEEP_LEN)
        n = self.scan_size()
        pop = np.zeros(n, dtype=np.int32) if want_points else None
        sig = np.zeros(n) if want_points else None
        self._chk(self._L.vxba_lio_sweep(self._h, _c(state), self._cov(cov), 1 if reset_cache else 0, out,
                                         _ptr(pop), _ptr(sig)))
        res = unpack_sweep(out)
        if want_points:
            res["plane_of_point"] = pop; res["sigma_of_point"] = sig
        return res

    def lio_state_estimation(self, state, cov):
        """Returns dict(ok, state, cov, iterations, match_num, min_eig, sweeps)."""
        st = _c(state).copy(); cv = self._cov(cov).copy()
        info = np.zeros(4); sweeps = np.zeros((LIO_MAX_ITER, LIO_SWEEP_LEN))
        self._chk(self._L.vxba_lio_state_estimation(self._h, st, cv, _ptr(info), _ptr(sweeps)))
        it = int(info[1])
        return {"ok": bool(info[0]), "state": st, "cov": cv.T.copy(), "iterations": it, "match_num": int(info[2]), "min_eig": float(info[3]),
                "sweeps": [unpack_sweep(sweeps[k]) for k in range(it)]}

    def pvec_update(self, state, cov, with_var: bool = True, resident: bool = False):
        """World points (and, unless ``with_var`` is False, world covariances n x 3 x 3) of the scan; both stay on the device for leaf_stats
        and LocalMap.cut_voxel_lio.  ``resident=True`` returns nothing: the result only stays on the device."""
        n = self.scan_size()
        if resident:
            self._chk(self._L.vxba_lio_pvec_update(self._h, _c(state), self._cov(cov), None, None))
            return None
        pw = np.zeros((n, 3))
        if not with_var:
            self._chk(self._L.vxba_lio_pvec_update(self._h, _c(state), self._cov(cov), _ptr(pw), None))
            return pw
        var = np.zeros((n, 9))
        self._chk(self._L.vxba_lio_pvec_update(self._h, _c(state), self._cov(cov), _ptr(pw), _ptr(var)))
        return pw, np.transpose(var.reshape(n, 3, 3), (0, 2, 1)).copy()

    def leaf_stats(self, cell_ptr, order):
        """Per-leaf increments of ``cut_voxel`` (OctoTree::push, voxel_map.hpp:969-993) from the resident world points / covariances of the
        last pvec_update: leaf c owns scan points ``order[cell_ptr[c]:cell_ptr[c+1]]``.  Returns clusters (n_cells x 10), cov_add (n_cells x 9 x 9)."""
        cp = np.ascontiguousarray(cell_ptr, dtype=np.int64); n = cp.shape[0] - 1
        od = np.ascontiguousarray(order, dtype=np.int32)
        if n < 0 or (n >= 0 and od.shape[0] != (cp[-1] if cp.size else 0)):
            raise VxbaError("leaf_stats: order must hold cell_ptr[-1] indices")
        cl = np.zeros((max(n, 0), 10)); ca = np.zeros((max(n, 0), 81))
        self._chk(self._L.vxba_lio_leaf_stats(self._h, n, cp, _ptr(od), cl, ca))
        return cl, ca.reshape(-1, 9, 9)          # symmetric: column-major == row-major, no transpose needed


class InitOdometry(_Handle):
    """The odometry of the first ``win_size`` scans on the GPU: ``lio_state_estimation_kdtree`` (voxelslam.cpp:960-1098) against a
    device-resident world cloud (``pl_tree``).  The five-nearest search is exact brute force in float32, equal distances to the lower index.
    States and covariances as in :class:`LioEstimator`."""
    _prefix = "vxba_initodom"
    NMATCH = 5

    def __init__(self, device: int = 0):
        self._create(int(device))

    def clear(self):
        """``pl_tree->clear()`` of ``system_reset``."""
        self._chk(self._L.vxba_initodom_clear(self._h))

    def cloud_size(self) -> int:
        return int(self._L.vxba_initodom_cloud_size(self._h))

    def cloud(self):
        """The resident cloud, n x 3 float32."""
        out = np.zeros((self.cloud_size(), 3), dtype=np.float32)
        self._chk(self._L.vxba_initodom_cloud(self._h, out))
        return out

    def search(self, queries):
        """The search alone: float32 queries n x 3 -> (idx n x 5 ascending by (distance, index), -1 beyond the cloud's size; sqd n x 5 float32)."""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 3)
        idx = np.zeros((q.shape[0], self.NMATCH), dtype=np.int32); sqd = np.zeros((q.shape[0], self.NMATCH), dtype=np.float32)
        self._chk(self._L.vxba_initodom_search(self._h, q.shape[0], q, idx, sqd))
        return idx, sqd

    def step(self, pnt_body, state, cov):
        """One scan.  Returns dict(seeded, state, cov, iterations, valid (per iteration), rematch_num, refind (per iteration), sweeps)."""
        pnt = _c(pnt_body).reshape(-1, 3)
        st = _c(state).copy(); cv = LioEstimator._cov(cov).copy()
        info = np.zeros(8); sweeps = np.zeros((LIO_MAX_ITER, LIO_SWEEP_LEN))
        self._chk(self._L.vxba_initodom_step(self._h, pnt.shape[0], pnt, st, cv, info, sweeps))
        it = int(info[1])
        sw = [unpack_sweep(sweeps[k]) for k in range(it)]
        return {"seeded": bool(info[0]), "state": st, "cov": cv.T.copy(), "iterations": it, "valid": [w["match_num"] for w in sw], "rematch_num": int(info[3]),
                "refind": [bool(info[4 + k]) for k in range(it)], "sweeps": sw}

    def inspect(self, iteration: int):
        """Per point of the last step's scan, as the search of ``iteration`` left it: dict(nn n x 5, ok n bool, n n x 3, d n)."""
        npts = self.stats()["scan_size"]
        nn = np.zeros((npts, self.NMATCH), dtype=np.int32); ok = np.zeros(npts, dtype=np.int32); pl = np.zeros((npts, 4))
        self._chk(self._L.vxba_initodom_inspect(self._h, int(iteration), nn, ok, pl))
        return {"nn": nn, "ok": ok.astype(bool), "n": pl[:, :3].copy(), "d": pl[:, 3].copy()}

    def stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self._L.vxba_initodom_stats(self._h, out))
        return {"launches": int(out[0]), "syncs": int(out[1]), "cloud_size": int(out[2]), "scan_size": int(out[3])}


class ImuEkf(_Handle):
    """``IMUEKF`` (ekf_imu.hpp): raw scan + raw IMU messages in, the IMU-propagated state and covariance, the de-skewed scan (device resident) and the
    edited message list for ``IMU_PRE.push_imu`` out.  Propagation on the host in f64, the de-skew in one kernel launch; the filtered cloud goes on
    to :meth:`LioEstimator.var_init_device` without leaving the device.  States and covariances as in :class:`LioEstimator`."""
    _prefix = "vxba_imuekf"
    MAX_HEADS = 64

    def __init__(self, params: "ImuEkfParams" = None, device: int = 0):
        self._create(int(device), None if params is None else C.byref(params))
        self.n_heads = 0

    def process(self, state, cov, scan, imus, beg_time, end_time):
        """``process()``.  scan: (xyz n x 3 float32 LiDAR frame, toff n float32 seconds after ``beg_time``, non-decreasing; None with point_notime);
        imus: (stamps K, gyr K x 3, acc K x 3).  Returns dict(ready, state, cov, imus (the edited list as a (stamps, gyr, acc) tuple, None while not
        ready), heads, compensated, point0_applications, t, scale_gravity, init_num)."""
        xyz = np.ascontiguousarray(scan[0], dtype=np.float32).reshape(-1, 3)
        toff = None if scan[1] is None else np.ascontiguousarray(scan[1], dtype=np.float32).reshape(-1)
        if toff is not None and toff.shape[0] != xyz.shape[0]:
            raise VxbaError("ImuEkf.process: toff must hold one value per point")
        st_, gy, ac = _c(imus[0]).reshape(-1), _c(imus[1]).reshape(-1, 3), _c(imus[2]).reshape(-1, 3)
        K = st_.shape[0]
        if gy.shape[0] != K or ac.shape[0] != K:
            raise VxbaError("ImuEkf.process: stamps, gyr and acc must hold the same number of messages")
        st = _c(state).reshape(STATE_LEN).copy(); cv = LioEstimator._cov(cov).copy()
        out = np.zeros((K + 1, 7)); info = np.zeros(8); k_out = C.c_int()
        self._chk(self._L.vxba_imuekf_process(self._h, xyz.shape[0], _ptr(xyz), _ptr(toff), K,
                                              st_ if K else np.zeros(1), gy if K else np.zeros(3), ac if K else np.zeros(3), float(beg_time), float(end_time), st, cv, out,
                                              C.byref(k_out), info))
        ready = bool(info[0])
        if ready:
            self.n_heads = int(info[1])
        return {"ready": ready, "state": st, "cov": cv.T.copy(), "imus": (out[:, 0].copy(), out[:, 1:4].copy(), out[:, 4:7].copy()) if ready else None,
                "heads": int(info[1]), "compensated": int(info[2]), "point0_applications": int(info[3]), "t": float(info[4]), "scale_gravity": float(info[5]),
                "init_num": int(info[6])}

    def process_device(self, state, cov, intake: "ScanIntake", imus, beg_time, end_time):
        """:meth:`process` with the scan taken from ``intake``'s resident cloud, device to device: the same dict, ``compensated`` -1."""
        st_, gy, ac = _c(imus[0]).reshape(-1), _c(imus[1]).reshape(-1, 3), _c(imus[2]).reshape(-1, 3)
        K = st_.shape[0]
        if gy.shape[0] != K or ac.shape[0] != K:
            raise VxbaError("ImuEkf.process_device: stamps, gyr and acc must hold the same number of messages")
        st = _c(state).reshape(STATE_LEN).copy(); cv = LioEstimator._cov(cov).copy()
        out = np.zeros((K + 1, 7)); info = np.zeros(8); k_out = C.c_int()
        self._chk(self._L.vxba_imuekf_process_device(self._h, intake._h, K, st_ if K else np.zeros(1), gy if K else np.zeros(3), ac if K else np.zeros(3), float(beg_time),
                                                     float(end_time), st, cv, out, C.byref(k_out), info))
        ready = bool(info[0])
        if ready:
            self.n_heads = int(info[1])
        return {"ready": ready, "state": st, "cov": cv.T.copy(), "imus": (out[:, 0].copy(), out[:, 1:4].copy(), out[:, 4:7].copy()) if ready else None,
                "heads": int(info[1]), "compensated": int(info[2]), "point0_applications": int(info[3]), "t": float(info[4]), "scale_gravity": float(info[5]),
                "init_num": int(info[6])}

    def stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self._L.vxba_imuekf_stats(self._h, out))
        return {"launches": int(out[0]), "waits": int(out[1]), "n": int(out[2]), "n_filtered": int(out[3])}

    def set_profiling(self, enable: bool):
        self._chk(self._L.vxba_imuekf_set_profiling(self._h, 1 if enable else 0))

    def stage_times(self):
        """Device milliseconds of the last process / filter from events on the handle's stream (waits for it): dict(deskew, filter); -1 where none ran."""
        out = np.zeros(2)
        self._chk(self._L.vxba_imuekf_stage_times(self._h, out))
        return {"deskew": float(out[0]), "filter": float(out[1])}

    def read_scan(self):
        """The de-skewed cloud, n x 3 float32, input order."""
        out = np.zeros((self.stats()["n"], 3), dtype=np.float32)
        self._chk(self._L.vxba_imuekf_read_scan(self._h, out))
        return out

    def pose_table(self):
        """``imu_poses`` of the last ready process: M x 22 rows [offt | R col-major | p | v | rate | acc_imu], the state before each step."""
        out = np.zeros((self.MAX_HEADS, 22))
        self._chk(self._L.vxba_imuekf_pose_table(self._h, out))
        return out[: self.n_heads].copy()

    def reinit(self, imus, scale):
        """``system_reset``'s share (voxelslam.cpp:1302-1305); returns the new gravity ``-mean_acc * scale``."""
        st_, gy, ac = _c(imus[0]).reshape(-1), _c(imus[1]).reshape(-1, 3), _c(imus[2]).reshape(-1, 3)
        g = np.zeros(3)
        self._chk(self._L.vxba_imuekf_reinit(self._h, st_.shape[0], st_ if st_.size else np.zeros(1), gy if gy.size else np.zeros(3), ac if ac.size else np.zeros(3), float(scale), g))
        return g

    def clear(self):
        self._chk(self._L.vxba_imuekf_clear(self._h))
        self.n_heads = 0

    def filter(self, down_size, min_points=500):
        """voxelslam.cpp:1574-1581 on the resident de-skewed cloud.  Returns (points kept, whether the half size was used)."""
        n = C.c_int64()
        self._chk(self._L.vxba_imuekf_filter(self._h, float(down_size), int(min_points), C.byref(n)))
        return int(n.value), self._L.vxba_imuekf_filter_passes(self._h) == 2

    def filtered(self):
        out = np.zeros((self.stats()["n_filtered"], 3), dtype=np.float32)
        self._chk(self._L.vxba_imuekf_filtered(self._h, out))
        return out

    def filtered_device(self):
        """(device pointer, n) of the filtered cloud, for :meth:`LioEstimator.var_init_device`."""
        p, n = C.c_void_p(), C.c_int64()
        self._chk(self._L.vxba_imuekf_filtered_device(self._h, C.byref(p), C.byref(n)))
        return p, int(n.value)


class ScanIntake(_Handle):
    """The handlers of ``Features::process`` (feature_point.hpp) and ``pcl_handler`` (voxelslam.hpp:76-103): the point bytes of a driver message in,
    the decimated, range-filtered, time-sorted and trimmed cloud out, resident for :meth:`ImuEkf.process_device`."""
    _prefix = "vxba_intake"
    REC = ("n_out", "toff_first", "toff_last", "fallback", "n_decoded", "n_filtered")

    def __init__(self, device: int = 0):
        self._create(int(device))
        self.n = 0

    def push(self, layout: "ScanLayout", data, point_filter_num=1, blind=1.0, time_head=0.0, n_points=None):
        """data: the message's point bytes (bytes, bytearray or a uint8 array), ``n_points`` x ``layout.point_step`` (None: all of them).  Returns
        dict(n_out, toff_first, toff_last, fallback, n_decoded, n_filtered, record (the six doubles as they came))."""
        return self._push(self._L.vxba_intake_push, "push", layout, data, point_filter_num, blind, time_head, n_points)

    def push_yaw(self, layout: "ScanLayout", data, point_filter_num=1, blind=1.0, omega_l=3610.0, n_points=None):
        """:meth:`push` for a ``RULE_YAW`` layout: every point's time from its yaw angle (feature_point.hpp:200-252), ``omega_l`` in degrees per
        second.  The same dict; :meth:`yaw_info` tells what the walk met."""
        return self._push(self._L.vxba_intake_push_yaw, "push_yaw", layout, data, point_filter_num, blind, omega_l, n_points)

    def _push(self, fn, who, layout, data, point_filter_num, blind, scalar, n_points):
        buf = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray, memoryview)) else np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
        step = int(layout.point_step)
        if n_points is None:
            if step < 1 or buf.shape[0] % step:
                raise VxbaError(f"ScanIntake.{who}: the data is not a whole number of points")
            n_points = buf.shape[0] // step
        elif int(n_points) > 0 and (step < 1 or int(n_points) * step > buf.shape[0]):
            raise VxbaError(f"ScanIntake.{who}: the data holds fewer than n_points points")
        rec = np.zeros(6)
        rc = fn(self._h, C.byref(layout), int(n_points), _ptr(buf) if buf.shape[0] else None, int(point_filter_num), float(blind), float(scalar), rec)
        self.last_record = rec                # readable after a refusal too: all zero when nothing ran
        if rc != 0 and rec[5] > 0:            # every survivor behind 0.11: reported after the run, the handle holds no cloud
            self.n = 0
        self._chk(rc)
        self.n = int(rec[0])
        return {"n_out": int(rec[0]), "toff_first": np.float32(rec[1]), "toff_last": np.float32(rec[2]), "fallback": bool(rec[3]), "n_decoded": int(rec[4]),
                "n_filtered": int(rec[5]), "record": rec}

    def yaw_info(self):
        """dict(skipped, active, candidates, events) of the last push when that was :meth:`push_yaw`; VxbaError (VXBA_ERR_STATE) otherwise."""
        out = np.zeros(4, dtype=np.int64)
        self._chk(self._L.vxba_intake_yaw_info(self._h, out))
        return {"skipped": int(out[0]), "active": int(out[1]), "candidates": int(out[2]), "events": int(out[3])}

    def read(self):
        """(xyz n x 3 float32, toff n float32) of the last push: by time, ties in input order."""
        xyz, toff = np.zeros((self.n, 3), dtype=np.float32), np.zeros(self.n, dtype=np.float32)
        self._chk(self._L.vxba_intake_read(self._h, xyz, toff))
        return xyz, toff

    def device(self):
        """(device pointer of xyz, of toff, n), valid until the next push."""
        px, pt, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._chk(self._L.vxba_intake_device(self._h, C.byref(px), C.byref(pt), C.byref(n)))
        return px, pt, int(n.value)

    def stats(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self._L.vxba_intake_stats(self._h, out))
        return {"launches": int(out[0]), "waits": int(out[1]), "n": int(out[2]), "n_decoded": int(out[3])}

    def set_profiling(self, enable: bool):
        self._chk(self._L.vxba_intake_set_profiling(self._h, 1 if enable else 0))

    def stage_times(self):
        """Device milliseconds of the last push (waits for the stream): dict(decode (upload + decode / filter), sort, push); -1 where none ran."""
        out = np.zeros(3)
        self._chk(self._L.vxba_intake_stage_times(self._h, out))
        return {"decode": float(out[0]), "sort": float(out[1]), "push": float(out[2])}


def init_pose_table(stamps, gyr, acc, beg_time, xc, bias_from, scale=1.0):
    """The IMU pose table of ``motion_blur`` (voxelslam.cpp:495-521): (K - 1) x 22 rows [offt | R col-major | p | v | rate | acc_imu], heads K-2 .. 0."""
    st = _c(stamps).reshape(-1)
    out = np.zeros((max(st.shape[0] - 1, 0), 22))
    rc = load_library().vxba_init_pose_table(st.shape[0], st, _c(gyr).reshape(-1, 3), _c(acc).reshape(-1, 3), float(beg_time), _c(xc), _c(bias_from), float(scale),
                                             out if out.size else np.zeros(22))
    if rc != 0:
        raise VxbaError(f"vxba_init_pose_table: {_ERRNAMES.get(rc, rc)}")
    return out


def init_deskew(xyz, toff, stamps, gyr, acc, beg_time, xc, bias_from, ext, scale=1.0, point_notime=False, device: int = 0):
    """``motion_blur`` (voxelslam.cpp:488-561) of one raw scan on the GPU.  Returns (points m x 3 float64 in upstream's output order, src m: the scan index
    of each): descending time, points at or before the earliest IMU offset dropped, the first point repeated under every earlier head it is later than.
    ``point_notime``: the extrinsic only, input order."""
    L = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    K = 0 if point_notime else int(np.asarray(stamps).reshape(-1).shape[0])
    cap = n + K + 1
    out = np.zeros((cap, 3)); src = np.zeros(cap, dtype=np.int32); m = C.c_int64()
    keep = []

    def ptr(a, dt=np.float64):
        if point_notime or a is None:
            return None
        arr = np.ascontiguousarray(a, dtype=dt); keep.append(arr)
        return _ptr(arr)
    rc = L.vxba_init_deskew(int(device), n, xyz, ptr(toff, np.float32), K, ptr(stamps), ptr(gyr), ptr(acc), float(beg_time), _c(xc), ptr(bias_from), _c(ext), float(scale),
                            1 if point_notime else 0, cap, out, src, C.byref(m))
    if rc != 0:
        raise VxbaError(f"vxba_init_deskew: {_ERRNAMES.get(rc, rc)}")
    return out[: m.value].copy(), src[: m.value].copy()


def init_normal_scatter(factor: "LidarFactor"):
    """Sum of n n^T over the plane normals in the factor's cache (``eig_vectors[k].col(0)``), 3 x 3: ``motion_init``'s degeneracy test."""
    out = np.zeros(9)
    rc = load_library().vxba_init_normal_scatter(factor._h, out)
    if rc != 0:
        raise VxbaError(f"vxba_init_normal_scatter: {_ERRNAMES.get(rc, rc)}")
    return out.reshape(3, 3).T.copy()


INIT_MAX_ROUNDS = 10
INIT_REPORT_LEN = 12


def motion_init(local_map: "LocalMap", factor: "LidarFactor", scans, beg_times, imus, states, covs, ext, imus_factor, noise_meas, noise_walk,
                min_eigen_value, plane_eigen_value_thre, imupre_scale_gravity=1.0, dept_err=0.02, beam_err=0.05, point_notime=False, imu_coef=1e-4):
    """``Initialization::motion_init`` (voxelslam.cpp:563-713) on the GPU.  ``scans``: W entries of (xyz n x 3 float32, toff n float32 seconds, ascending);
    ``imus``: W entries of (stamps, gyr, acc), the raw messages of each scan's interval; ``states`` W x 24, ``covs`` W x 15 x 15; ``imus_factor`` the W - 1
    ``IMU_PRE`` (rebuilt in place); ``min_eigen_value`` / ``plane_eigen_value_thre``: the caller's plane thresholds (the map must have been created with
    ``thread_num=1``).  Returns dict(flag, states, hess, rounds: per round dict(n_vox, resis, g, ratio, phase, n_iter, solved, thre, fired, trace), eig)."""
    L = load_library()
    W = factor.win_size
    sp = np.zeros(W + 1, dtype=np.int64); ip = np.zeros(W + 1, dtype=np.int64)
    for i in range(W):
        sp[i + 1] = sp[i] + np.asarray(scans[i][0]).reshape(-1, 3).shape[0]
        ip[i + 1] = ip[i] + np.asarray(imus[i][0]).reshape(-1).shape[0]
    xyz = np.ascontiguousarray(np.concatenate([np.asarray(s[0], dtype=np.float32).reshape(-1, 3) for s in scans]) if sp[W] else np.zeros((1, 3)), dtype=np.float32)
    toff = None if point_notime else np.ascontiguousarray(np.concatenate([np.asarray(s[1], dtype=np.float32).reshape(-1) for s in scans]) if sp[W] else np.zeros(1), dtype=np.float32)
    st = _c(np.concatenate([np.asarray(m[0], dtype=np.float64).reshape(-1) for m in imus]))
    gy = _c(np.concatenate([np.asarray(m[1], dtype=np.float64).reshape(-1, 3) for m in imus]))
    ac = _c(np.concatenate([np.asarray(m[2], dtype=np.float64).reshape(-1, 3) for m in imus]))
    x = _c(states).reshape(W, STATE_LEN).copy()
    cv = np.ascontiguousarray(np.transpose(np.asarray(covs, dtype=np.float64).reshape(W, 15, 15), (0, 2, 1)))
    prm = InitMotionParams(float(imupre_scale_gravity), float(dept_err), float(beam_err), float(imu_coef),
                           (C.c_double * 36)(*np.asarray(noise_meas, dtype=np.float64).T.reshape(-1)), (C.c_double * 36)(*np.asarray(noise_walk, dtype=np.float64).T.reshape(-1)),
                           float(min_eigen_value), (C.c_double * 4)(*plane_eigen_value_thre), 1 if point_notime else 0)
    blobs = LI_BA_Optimizer._blobs(imus_factor).copy()
    n = LI_DIM * W + 3
    hess = np.zeros((n, n)); report = np.zeros((INIT_MAX_ROUNDS, INIT_REPORT_LEN)); traces = np.zeros((INIT_MAX_ROUNDS, 3, TRACE_COLS))
    nr = C.c_int(0); flag = C.c_int(0); eig = np.zeros(3)
    rc = L.vxba_init_motion(local_map._h, factor.handle, W, sp, xyz, _ptr(toff), _c(beg_times), ip, st, gy, ac, x, cv,
                            _c(ext), C.byref(prm), blobs, hess, report, traces, C.byref(nr), eig, C.byref(flag))
    if rc != 0:
        raise VxbaError(f"vxba_init_motion: {_ERRNAMES.get(rc, rc)}: {(L.vxba_map_last_error(local_map._h) or b'').decode()} {(L.vxba_last_error(factor.handle) or b'').decode()}")
    for f, b in zip(imus_factor, blobs):
        f.blob[:] = b
    rounds = []
    for k in range(nr.value):
        r = report[k]
        ni = int(r[8])
        rounds.append(dict(n_vox=int(r[0]), resis=r[1:3].copy(), g=r[3:6].copy(), ratio=float(r[6]), phase=int(r[7]), n_iter=ni, solved=bool(r[9]), thre=float(r[10]),
                           fired=bool(r[11]), trace=traces[k, :ni].copy()))
    us = np.zeros(4)
    L.vxba_init_motion_times(us)
    return dict(flag=flag.value, states=x, hess=hess.T, rounds=rounds, eig=eig, stage_ms=dict(zip(("deskew", "map_build", "lm", "repreintegration"), us / 1e3)))


def down_sampling_voxel(xyz, voxel_size: float, device: int = 0):
    """``down_sampling_voxel`` (tools.hpp:201-238) on float32 points; one point per occupied voxel, ascending voxel index."""
    L = load_library()
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(xyz)
    n_out = C.c_int64()
    rc = L.vxba_down_sampling_voxel(device, xyz.shape[0], xyz, float(voxel_size), out, C.byref(n_out))
    if rc != 0:
        raise VxbaError(f"vxba_down_sampling_voxel: {_ERRNAMES.get(rc, rc)}")
    return out[: n_out.value].copy()


def down_sampling_close(xyz, voxel_size: float, device: int = 0):
    """``down_sampling_close`` (tools.hpp:240-302) on the GPU: per occupied voxel the point nearest the voxel's mean.  Returns (points m x 3 float32 in
    ascending voxel index, sel m: their indices into ``xyz``)."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
    out = np.zeros_like(xyz); sel = np.zeros(max(xyz.shape[0], 1), dtype=np.int32); m = C.c_int64()
    rc = load_library().vxba_down_sampling_close(int(device), xyz.shape[0], xyz, float(voxel_size), out, sel, C.byref(m))
    if rc != 0:
        raise VxbaError(f"vxba_down_sampling_close: {_ERRNAMES.get(rc, rc)}")
    return out[: m.value].copy(), sel[: m.value].copy()


def voxelize_profile(enable: bool):
    """``vxba_voxelize_profile``: start (True) or stop (False -> dict(ms_sum, launches, algorithmic_bytes)) the measurement of the
    cluster-build kernel inside the voxeliser."""
    L = load_library()
    ms, n, b = C.c_double(), C.c_longlong(), C.c_double()
    L.vxba_voxelize_profile(1 if enable else 0, C.byref(ms), C.byref(n), C.byref(b))
    return None if enable else dict(ms_sum=ms.value, launches=int(n.value), algorithmic_bytes=b.value)


class HbaSession:
    """``vxba_hba_*``: a session of keyframes resident on the device and the bottom-up pass of the hierarchical global BA over it
    (thd_globalmapping / HBA_add_edge, voxelslam.cpp:2485-2595, 2320-2482) below the C ABI -- see csrc/vxba_hba.hip.  The Python twin that
    orchestrates the same calls window by window (and runs on the CPU oracle in the tests) is ``voxel_slam_amd.hba.hierarchical_ba``."""

    def __init__(self, device: int = 0):
        L = load_library()
        L.vxba_hba_last_error.restype = C.c_char_p
        self._L = L
        self._h = C.c_void_p()
        rc = L.vxba_hba_create(int(device), C.byref(self._h))
        if rc != 0:
            raise VxbaError(f"vxba_hba_create: {_ERRNAMES.get(rc, rc)}")

    def close(self):
        if getattr(self, "_h", None):
            self._L.vxba_hba_destroy(self._h)
            self._h = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise VxbaError(f"{what}: {_ERRNAMES.get(rc, rc)}: {self._L.vxba_hba_last_error(self._h).decode()}")

    def add_keyframes(self, clouds):
        """clouds: list of (n_i, 3) arrays in keyframe coordinates (stored as float32, like PointType)."""
        ptr = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int64)
        xyz = np.ascontiguousarray(np.concatenate([np.asarray(c, dtype=np.float32).reshape(-1, 3) for c in clouds])) if len(clouds) else np.zeros((0, 3), np.float32)
        self._check(self._L.vxba_hba_add_keyframes(self._h, C.c_int64(len(clouds)), ptr.ctypes.data_as(C.c_void_p), xyz.ctypes.data_as(C.c_void_p)), "vxba_hba_add_keyframes")

    def add_keyframes_device(self, sizes, d_xyz: int):
        """The same from device memory: ``sizes`` points per cloud, ``d_xyz`` the raw device address of the clouds back to back, (sum sizes, 3) float32."""
        ptr = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64).reshape(-1))]).astype(np.int64)
        self._check(self._L.vxba_hba_add_keyframes_device(self._h, C.c_int64(ptr.size - 1), ptr.ctypes.data_as(C.c_void_p), C.c_void_p(int(d_xyz) if d_xyz else None)),
                    "vxba_hba_add_keyframes_device")

    def num_keyframes(self) -> int:
        return int(self._L.vxba_hba_num_keyframes(self._h))

    def device_clouds(self):
        """(raw device address of the packed clouds (0: no point), cloud_ptr (K + 1,) int64 copy): a set of ``global_map``; the address is valid
        until the next add_keyframes / clear."""
        d, p, k = C.c_void_p(), C.c_void_p(), C.c_int64()
        self._check(self._L.vxba_hba_device_clouds(self._h, C.byref(d), C.byref(p), C.byref(k)), "vxba_hba_device_clouds")
        ptr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int64)), shape=(int(k.value) + 1,)).copy()
        return d.value or 0, ptr

    def clear(self):
        self._check(self._L.vxba_hba_clear(self._h), "vxba_hba_clear")

    @staticmethod
    def windows(K: int, wdsize: int, mgsize: int, tail: bool = True):
        """``vxba_hba_num_windows`` / ``vxba_hba_window``: [(first keyframe, keyframe count)] of a pass over K keyframes -- the full windows at stride
        ``mgsize`` and, with ``tail``, the closing short window of upstream's last iteration (voxelslam.cpp:2519-2523)."""
        L = load_library()
        n = L.vxba_hba_num_windows(int(K), int(wdsize), int(mgsize), int(bool(tail)))
        out = []
        for w in range(n):
            f0, c = C.c_int(), C.c_int()
            L.vxba_hba_window(int(K), int(wdsize), int(mgsize), int(bool(tail)), w, C.byref(f0), C.byref(c))
            out.append((f0.value, c.value))
        return out

    @staticmethod
    def _edges(eij, edata, lo, hi, win=None):
        return [dict(i=int(eij[k, 0]), j=int(eij[k, 1]), rot=edata[k, :9].reshape(3, 3).copy(), tra=edata[k, 9:12].copy(), v6=edata[k, 12:18].copy(),
                     **({} if win is None else {"window": int(win[k])})) for k in range(lo, hi)]

    def _poses(self, poses):
        poses = _c(poses).reshape(-1, 12)
        if poses.shape[0] != self.num_keyframes():
            raise VxbaError(f"hba pass: {poses.shape[0]} poses for {self.num_keyframes()} keyframes")
        return poses

    def run_pass(self, poses, coarse: VoxelizeParams, fine: VoxelizeParams, wdsize: int = 10, mgsize: int = 5, top_max_iter: int = 1, n_threads: int = 0,
                 tail: bool = True):
        """One bottom-up pass on this device (``vxba_hba_pass``); returns what ``hba.hierarchical_ba`` returns (edges as dicts with keyframe indices)."""
        poses = self._poses(poses)
        K = poses.shape[0]
        wins = self.windows(K, wdsize, mgsize, tail)
        S = len(wins)
        if S < 1:
            raise VxbaError(f"hba pass: no window for {K} keyframes with wdsize {wdsize}, mgsize {mgsize}, tail {tail}")
        cap = sum(c * (c - 1) // 2 for _, c in wins) + S * (S - 1) // 2 + 1
        sub_poses = np.zeros((S, 12)); sizes = np.zeros(S, dtype=np.int64)
        eij = np.zeros((cap, 2), dtype=np.int32); edata = np.zeros((cap, 18))
        n1, n2, ntr = C.c_int64(), C.c_int64(), C.c_int()
        rounds = np.zeros((max(1, top_max_iter), 5))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._L.vxba_hba_pass(self._h, vp(poses), C.byref(coarse), C.byref(fine), int(wdsize), int(mgsize), int(bool(tail)), int(top_max_iter), int(n_threads),
                                          vp(sub_poses), vp(sizes), C.c_int64(cap), vp(eij), vp(edata), C.byref(n1), C.byref(n2), vp(rounds), C.byref(ntr)), "vxba_hba_pass")
        return dict(edges1=self._edges(eij, edata, 0, n1.value), edges2=self._edges(eij, edata, n1.value, n1.value + n2.value), submap_ids=[f0 for f0, _ in wins],
                    submap_poses=sub_poses, submap_sizes=[int(x) for x in sizes], n_threads_used=int(self._L.vxba_hba_threads_used(self._h)),
                    top_rounds=self._rounds(rounds, ntr.value))

    @staticmethod
    def _rounds(rounds, n):
        return [dict(round=k, n_voxels=int(rounds[k, 0]), resis=(float(rounds[k, 1]), float(rounds[k, 2])), converged=bool(rounds[k, 3]), fine=bool(rounds[k, 4])) for k in range(n)]

    # ---- the pass in its two halves (one rank of N: voxel_slam_amd.dist.hba_pass) ----
    def bottom(self, poses, coarse: VoxelizeParams, fine: VoxelizeParams, wdsize: int = 10, mgsize: int = 5, tail: bool = True, w_first: int = 0, w_stride: int = 1,
               n_threads: int = 0):
        """``vxba_hba_bottom``: the windows w_first, w_first + w_stride, .. on this device.  Returns dict(sizes (S, -1 where not run here), edges (dicts with
        ``window``), windows)."""
        poses = self._poses(poses)
        wins = self.windows(poses.shape[0], wdsize, mgsize, tail)
        S = len(wins)
        cap = sum(c * (c - 1) // 2 for _, c in wins[w_first::w_stride]) + 1
        sub_poses = np.zeros((S, 12)); sizes = np.full(S, -1, dtype=np.int64)
        eij = np.zeros((cap, 2), dtype=np.int32); edata = np.zeros((cap, 18)); ewin = np.zeros(cap, dtype=np.int32)
        ne = C.c_int64()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._last_geom = (poses.shape[0], int(wdsize), int(mgsize), int(bool(tail)))
        self._check(self._L.vxba_hba_bottom(self._h, vp(poses), C.byref(coarse), C.byref(fine), int(wdsize), int(mgsize), int(bool(tail)), int(w_first), int(w_stride),
                                            int(n_threads), vp(sub_poses), vp(sizes), C.c_int64(cap), vp(eij), vp(edata), vp(ewin), C.byref(ne)), "vxba_hba_bottom")
        return dict(sizes=sizes, edges=self._edges(eij, edata, 0, ne.value, ewin), windows=wins, n_threads_used=int(self._L.vxba_hba_threads_used(self._h)))

    def export_submaps(self, w_first: int, w_stride: int, d_ptr: int, capacity_points: int) -> int:
        """``vxba_hba_export_submaps``: this selection's submaps packed into the DEVICE buffer at ``d_ptr`` (float xyz); returns the point count."""
        n = C.c_int64()
        self._check(self._L.vxba_hba_export_submaps(self._h, int(w_first), int(w_stride), C.c_void_p(d_ptr), C.c_int64(capacity_points), C.byref(n)), "vxba_hba_export_submaps")
        return int(n.value)

    def import_submaps(self, w_first: int, w_stride: int, sizes, d_ptr: int):
        """``vxba_hba_import_submaps``: a peer's packed submaps (DEVICE pointer) into place; ``sizes``: S entries."""
        sizes = np.ascontiguousarray(sizes, dtype=np.int64)
        self._check(self._L.vxba_hba_import_submaps(self._h, int(w_first), int(w_stride), sizes.ctypes.data_as(C.c_void_p), C.c_void_p(d_ptr)), "vxba_hba_import_submaps")

    def top_factor(self) -> "LidarFactor":
        """``vxba_hba_top_factor``: the (session-owned) factor the top level runs on, to attach a collective to."""
        h = C.c_void_p()
        self._check(self._L.vxba_hba_top_factor(self._h, C.byref(h)), "vxba_hba_top_factor")
        return LidarFactor.from_handle(h)

    def top(self, poses, coarse: VoxelizeParams, fine: VoxelizeParams, top_max_iter: int = 1):
        """``vxba_hba_top``: the top level over all submaps of the pass in progress.  Returns dict(submap_poses, edges2, top_rounds)."""
        poses = self._poses(poses)
        S = self._L.vxba_hba_num_windows(*self._geom(poses.shape[0]))
        cap = S * (S - 1) // 2 + 1
        sub_poses = np.zeros((S, 12))
        eij = np.zeros((cap, 2), dtype=np.int32); edata = np.zeros((cap, 18))
        ne, ntr = C.c_int64(), C.c_int()
        rounds = np.zeros((max(1, top_max_iter), 5))
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        self._check(self._L.vxba_hba_top(self._h, vp(poses), C.byref(coarse), C.byref(fine), int(top_max_iter), vp(sub_poses), C.c_int64(cap), vp(eij), vp(edata), C.byref(ne),
                                         vp(rounds), C.byref(ntr)), "vxba_hba_top")
        return dict(submap_poses=sub_poses, edges2=self._edges(eij, edata, 0, ne.value), top_rounds=self._rounds(rounds, ntr.value))

    def _geom(self, K):
        g = getattr(self, "_last_geom", None)
        if not g or g[0] != K:
            raise VxbaError("hba top: no pass in progress (HbaSession.bottom first)")
        return g


class PgoOptions(C.Structure):
    """vxba_pgo_options (include/vxba.h); a field left at 0 (rel_cost_tol: below 0) takes the library's default."""
    _fields_ = [("max_iter", C.c_int), ("cg_max_iter", C.c_int), ("cg_tol", C.c_double), ("rel_cost_tol", C.c_double), ("u0", C.c_double), ("v0", C.c_double)]

    def __init__(self, max_iter=0, cg_max_iter=0, cg_tol=0.0, rel_cost_tol=-1.0, u0=0.0, v0=0.0):
        super().__init__(int(max_iter), int(cg_max_iter), float(cg_tol), float(rel_cost_tol), float(u0), float(v0))


PGO_REPORT_LEN = 8


class PoseGraph(_Handle):
    """``vxba_pgo_*``: poses on SE(3) under between and prior factors with diagonal variances, optimised on the GPU (Levenberg-Marquardt around a
    block-Jacobi preconditioned CG whose loop stays on the device) -- what the reference hands to GTSAM's ISAM2 in topDownProcess and after a loop
    closure.  See include/vxba.h for the residuals, the chart and what is and is not pinned."""
    _prefix = "vxba_pgo"

    def __init__(self, poses=None, device: int = 0):
        self._create(int(device))
        if poses is not None:
            self.set_poses(poses)

    def clear(self):
        self._check(self._L.vxba_pgo_clear(self._h), "vxba_pgo_clear")

    def num_nodes(self) -> int:
        return int(self._L.vxba_pgo_num_nodes(self._h))

    def num_factors(self) -> int:
        return int(self._L.vxba_pgo_num_factors(self._h))

    def set_poses(self, poses):
        poses = _c(poses).reshape(-1, 12)
        self._check(self._L.vxba_pgo_set_poses(self._h, poses.shape[0], poses), "vxba_pgo_set_poses")

    def read_poses(self):
        out = np.zeros((self.num_nodes(), 12))
        self._check(self._L.vxba_pgo_read_poses(self._h, out), "vxba_pgo_read_poses")
        return out

    def add_edges(self, edge_ij, edge_data, node_offset_i: int = 0, node_offset_j: int = 0):
        """``edge_ij`` (n, 2) ints and ``edge_data`` (n, 18) -- the arrays ``vxba_hba_pass`` fills -- or, with ``edge_data`` None, a list of the edge
        dicts (i, j, rot, tra, v6) that ``hba.hierarchical_ba`` / ``HbaSession.run_pass`` return."""
        if edge_data is None:
            edge_ij, edge_data = pack_edges(edge_ij)
        ij = np.ascontiguousarray(edge_ij, dtype=np.int32).reshape(-1, 2)
        data = _c(edge_data).reshape(-1, 18)
        if ij.shape[0] != data.shape[0]:
            raise VxbaError(f"add_edges: {ij.shape[0]} index pairs for {data.shape[0]} records")
        self._check(self._L.vxba_pgo_add_edges(self._h, C.c_int64(ij.shape[0]), int(node_offset_i), int(node_offset_j), ij, data), "vxba_pgo_add_edges")

    def add_priors(self, nodes, poses12, v6):
        nodes = np.ascontiguousarray(np.atleast_1d(nodes), dtype=np.int32)
        poses12 = _c(poses12).reshape(-1, 12)
        v6 = np.ascontiguousarray(np.broadcast_to(_c(v6).reshape(-1, 6), (nodes.size, 6)))
        if poses12.shape[0] != nodes.size:
            raise VxbaError(f"add_priors: {nodes.size} nodes for {poses12.shape[0]} poses")
        self._check(self._L.vxba_pgo_add_priors(self._h, C.c_int64(nodes.size), nodes, poses12, v6), "vxba_pgo_add_priors")

    def cost(self, want_residuals: bool = False):
        """Cost at the current poses; with ``want_residuals`` also the (factors, 6) residuals in the order the factors were added."""
        c = C.c_double()
        res = np.zeros((self.num_factors(), 6)) if want_residuals else None
        self._check(self._L.vxba_pgo_cost(self._h, C.byref(c), _ptr(res)), "vxba_pgo_cost")
        return (c.value, res) if want_residuals else c.value

    def optimize(self, options: "PgoOptions | None" = None, **kw):
        """``vxba_pgo_optimize``; keyword arguments build a ``PgoOptions``.  Returns dict(poses, report, launches, host_syncs): one report entry per
        outer iteration -- cost_before, cost_after, accepted, u, cg_iterations, cg_capped, predicted_decrease, cg_residual."""
        opt = options if options is not None else PgoOptions(**kw)
        K = self.num_nodes()
        cap = opt.max_iter if opt.max_iter > 0 else 6
        poses = np.zeros((K, 12)); rep = np.zeros((cap, PGO_REPORT_LEN)); n = C.c_int()
        self._check(self._L.vxba_pgo_optimize(self._h, C.cast(C.byref(opt), C.c_void_p), _ptr(poses), _ptr(rep), cap, C.byref(n)), "vxba_pgo_optimize")
        st = np.zeros(4, dtype=np.int64)
        self._L.vxba_pgo_stats(self._h, st)
        report = [dict(cost_before=float(r[0]), cost_after=float(r[1]), accepted=bool(r[2]), u=float(r[3]), cg_iterations=int(r[4]), cg_capped=bool(r[5]),
                       predicted_decrease=float(r[6]), cg_residual=float(r[7])) for r in rep[:n.value]]
        return dict(poses=poses, report=report, launches=int(st[0]), host_syncs=int(st[1]))


class PlaneCloudParams(C.Structure):
    """vxba_planecloud_params (include/vxba.h): the voxel grid and plane test of STDescManager::init_voxel_map / BTCOctoTree::init_plane."""
    _fields_ = [("voxel_size", C.c_double), ("voxel_init_num", C.c_int), ("plane_detection_thre", C.c_double)]

    def __init__(self, voxel_size=1.0, voxel_init_num=10, plane_detection_thre=0.01):
        super().__init__(float(voxel_size), int(voxel_init_num), float(plane_detection_thre))


ICP_GATES0 = (0.2, 0.2, 0.5, 3.0)     # loop_refine.hpp:62
ICP_GATES1 = (0.1, 0.1, 0.1, 1.0)     # loop_refine.hpp:127
ICP_REPORT_LEN = 8


class IcpOptions(C.Structure):
    """vxba_icp_options (include/vxba.h); the defaults are icp_normal's (loop_refine.hpp:47-145) and voxelslam.cpp:1812's icp_eigval."""
    _fields_ = [("max_iter", C.c_int), ("gates0", C.c_double * 4), ("gates1", C.c_double * 4), ("step_tol", C.c_double), ("icp_eigval", C.c_double)]

    def __init__(self, max_iter=20, gates0=ICP_GATES0, gates1=ICP_GATES1, step_tol=1e-3, icp_eigval=14.0):
        super().__init__(int(max_iter), (C.c_double * 4)(*gates0), (C.c_double * 4)(*gates1), float(step_tol), float(icp_eigval))


class LoopRegistration(_Handle):
    """``vxba_loopreg_*``: device-resident plane clouds (n x 6 float32: centre, normal), the verify score of pose hypotheses
    (plane_geometric_verify) and the normal-gated point-to-plane ICP (icp_normal), batched over pairs.  A pose maps source-frame coordinates
    into the target frame.  See include/vxba.h for the arithmetic that is pinned bit for bit."""
    _prefix = "vxba_loopreg"

    def __init__(self, device: int = 0):
        self._create(int(device))

    def clear(self):
        self._check(self._L.vxba_loopreg_clear(self._h), "vxba_loopreg_clear")

    def num_clouds(self) -> int:
        return int(self._L.vxba_loopreg_num_clouds(self._h))

    def cloud_size(self, cloud_id: int) -> int:
        return int(self._L.vxba_loopreg_cloud_size(self._h, int(cloud_id)))

    def read_cloud(self, cloud_id: int):
        n = self.cloud_size(cloud_id)
        out = np.zeros((max(n, 0), 6), dtype=np.float32)
        self._check(self._L.vxba_loopreg_read_cloud(self._h, int(cloud_id), _ptr(out)), "vxba_loopreg_read_cloud")
        return out

    def add_cloud(self, xyzn) -> int:
        """A plane cloud as it is, (n, 6) float32 (x, y, z, nx, ny, nz); returns its id."""
        a = np.ascontiguousarray(xyzn, dtype=np.float32).reshape(-1, 6)
        cid = C.c_int()
        self._check(self._L.vxba_loopreg_add_cloud(self._h, C.c_int64(a.shape[0]), _ptr(a), C.byref(cid)), "vxba_loopreg_add_cloud")
        return cid.value

    def add_keyframe(self, xyz, params: "PlaneCloudParams | None" = None) -> int:
        """The plane cloud of a keyframe cloud (n, 3) in the keyframe's frame; returns its id (``cloud_size`` / ``read_cloud`` for the planes)."""
        a = _c(xyz).reshape(-1, 3)
        prm = params if params is not None else PlaneCloudParams()
        cid = C.c_int(); npl = C.c_int64()
        self._check(self._L.vxba_loopreg_add_keyframe(self._h, C.c_int64(a.shape[0]), _ptr(a), C.cast(C.byref(prm), C.c_void_p), C.byref(cid), C.byref(npl)),
                    "vxba_loopreg_add_keyframe")
        return cid.value

    def add_keyframe_device(self, n_points: int, d_xyz: int, params: "PlaneCloudParams | None" = None) -> int:
        """The same from a float32 cloud (n_points, 3) in device memory (raw address, e.g. ``KeyframeBuilder.device_ptrs()["full"]``): widened exactly,
        so the plane cloud is the one ``add_keyframe`` gives for the same floats."""
        prm = params if params is not None else PlaneCloudParams()
        cid = C.c_int(); npl = C.c_int64()
        self._check(self._L.vxba_loopreg_add_keyframe_device(self._h, C.c_int64(int(n_points)), _dev(d_xyz), C.cast(C.byref(prm), C.c_void_p), C.byref(cid),
                                                             C.byref(npl)), "vxba_loopreg_add_keyframe_device")
        return cid.value

    def stats(self):
        st = np.zeros(4, dtype=np.int64)
        self._L.vxba_loopreg_stats(self._h, st)
        return dict(launches=int(st[0]), host_syncs=int(st[1]), clouds=int(st[2]), pairs=int(st[3]))

    def associate(self, src: int, tar: int, pose, gates=ICP_GATES0):
        """Per source row: (nearest target index, gate verdict) under one hypothesis and one gate vector."""
        S = max(self.cloud_size(src), 0)
        nn = np.zeros(S, dtype=np.int32); m = np.zeros(S, dtype=np.uint8)
        self._check(self._L.vxba_loopreg_associate(self._h, int(src), int(tar), _c(pose).reshape(12), _c(gates).reshape(4), _ptr(nn), _ptr(m)),
                    "vxba_loopreg_associate")
        return nn, m.astype(bool)

    @staticmethod
    def _pairs(src_tar, poses):
        st = np.ascontiguousarray(src_tar, dtype=np.int32).reshape(-1, 2)
        P = np.array(poses, dtype=np.float64).reshape(-1, 12)
        if st.shape[0] != P.shape[0]:
            raise VxbaError(f"{st.shape[0]} cloud pairs for {P.shape[0]} poses")
        return st, np.ascontiguousarray(P)

    def score(self, src_tar, poses, normal_threshold=0.2, dis_threshold=0.5):
        """``plane_geometric_verify`` of every hypothesis: (score (B,), useful (B,) int64)."""
        st, P = self._pairs(src_tar, poses)
        B = st.shape[0]
        sc = np.zeros(B); us = np.zeros(B, dtype=np.int64)
        if B:
            self._check(self._L.vxba_loopreg_score(self._h, B, st, P, float(normal_threshold), float(dis_threshold), sc, us), "vxba_loopreg_score")
        return sc, us

    def icp(self, src_tar, poses, options: "IcpOptions | None" = None, **kw):
        """``icp_normal`` of every pair in one call; keyword arguments build an ``IcpOptions``.  Returns dict(poses (B, 12), report (B, 8), accept,
        is_converge, iterations, match_num, eig (B, 3), resi, launches, host_syncs)."""
        opt = options if options is not None else IcpOptions(**kw)
        st, P = self._pairs(src_tar, poses)
        B = st.shape[0]
        rep = np.zeros((B, ICP_REPORT_LEN))
        if B:
            self._check(self._L.vxba_loopreg_icp(self._h, B, st, P, C.cast(C.byref(opt), C.c_void_p), rep), "vxba_loopreg_icp")
        s = self.stats() if B else dict(launches=0, host_syncs=0)
        return dict(poses=P, report=rep, accept=rep[:, 0] > 0, is_converge=rep[:, 1] > 0, iterations=rep[:, 2].astype(np.int64), match_num=rep[:, 3].astype(np.int64),
                    eig=rep[:, 4:7], resi=rep[:, 7], launches=s["launches"], host_syncs=s["host_syncs"])


@dataclasses.dataclass
class LoopSearchParams:
    """vxba_loopsearch_params (include/vxba.h); the defaults are BTC.cpp:22-34's."""
    descriptor_near_num: int = 15
    descriptor_min_len: float = 2.0
    descriptor_max_len: float = 50.0
    std_side_resolution: float = 0.2
    skip_near_num: int = 30
    candidate_num: int = 20
    rough_dis_threshold: float = 0.01
    similarity_threshold: float = 0.7
    icp_threshold: float = 0.15
    normal_threshold: float = 0.2
    dis_threshold: float = 0.5

    class _C(C.Structure):
        _fields_ = [("descriptor_near_num", C.c_int), ("descriptor_min_len", C.c_double), ("descriptor_max_len", C.c_double), ("std_side_resolution", C.c_double),
                    ("skip_near_num", C.c_int), ("candidate_num", C.c_int), ("rough_dis_threshold", C.c_double), ("similarity_threshold", C.c_double),
                    ("icp_threshold", C.c_double), ("normal_threshold", C.c_double), ("dis_threshold", C.c_double)]

    def as_c(self):
        return self._C(*[getattr(self, f.name) for f in dataclasses.fields(self)])

    @classmethod
    def library_defaults(cls):
        """What ``vxba_loopsearch_default_params`` fills in (the tests compare it with the dataclass defaults)."""
        c = cls._C()
        load_library().vxba_loopsearch_default_params(C.cast(C.byref(c), C.c_void_p))
        return cls(*[getattr(c, f.name) for f in dataclasses.fields(cls)])


LOOPSEARCH_MAX_CORNERS = 2048
LOOPSEARCH_MAX_SESSIONS = 16


def pack_occupancy(occupancy):
    """Occupancy words of n corners as uint64: an integer array is taken as it is, a boolean (n, bits) array is packed bit k = column k.  More than
    64 bits per corner cannot be held in a word: VxbaError (VXBA_ERR_ARG), nothing launched."""
    a = np.asarray(occupancy)
    if a.dtype == np.bool_:
        a = a.reshape(a.shape[0], -1) if a.ndim >= 2 else a.reshape(-1, 1)
        if a.shape[1] > 64:
            raise VxbaError(f"pack_occupancy: VXBA_ERR_ARG: an occupancy of {a.shape[1]} bits does not fit the 64-bit word of a corner")
        return (a.astype(np.uint64) << np.arange(a.shape[1], dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    if a.dtype == object or a.dtype.kind not in "iu":
        vals = [int(v) for v in a.reshape(-1)]
        if any(v < 0 or v >> 64 for v in vals):
            raise VxbaError("pack_occupancy: VXBA_ERR_ARG: an occupancy word needs more than 64 bits")
        return np.array(vals, dtype=np.uint64)
    if a.dtype.kind == "i" and (a < 0).any():
        raise VxbaError("pack_occupancy: VXBA_ERR_ARG: an occupancy word is negative")
    return np.ascontiguousarray(a.reshape(-1), dtype=np.uint64)


class LoopSearch(_Handle):
    """``vxba_loopsearch_*``: the triangle descriptors of a keyframe's corners, the device-resident database of them and the search over it
    (generate_std, AddSTDescs, candidate_selector, candidate_verify, SearchLoop).  Attached to the ``LoopRegistration`` whose plane clouds the verify
    score reads.  Call order per keyframe: ``describe`` -> ``search`` -> ``add``.  See include/vxba.h for the arithmetic that is pinned."""

    _prefix = "vxba_loopsearch"
    CAND_INTS = 7
    CAND_DOUBLES = 13

    def __init__(self, reg: "LoopRegistration", device: int = 0):
        self._reg = reg                        # keeps the registration handle alive
        self.cloud_ids = []                    # frame -> the plane cloud it was added with
        self._create(int(device), reg._h)

    def close(self):
        if not self._reg._h:                   # the handle shares the registration's stream: gone with it, nothing left to destroy
            self._h = C.c_void_p()
        super().close()

    def clear(self):
        self._check(self._L.vxba_loopsearch_clear(self._h), "vxba_loopsearch_clear")
        self.cloud_ids = []

    def num_frames(self) -> int:
        return int(self._L.vxba_loopsearch_num_frames(self._h))

    def num_descriptors(self, which: int = -1) -> int:
        """Descriptors of frame ``which``; -1: of the database; -2: of the current set."""
        return int(self._L.vxba_loopsearch_num_descriptors(self._h, int(which)))

    def describe(self, locations, occupancy, params: "LoopSearchParams | None" = None) -> int:
        """Builds the current keyframe's descriptors from its corners -- locations (n, 3), occupancy n words (``pack_occupancy``); returns their count."""
        loc = _c(locations).reshape(-1, 3)
        occ = pack_occupancy(occupancy)
        if occ.shape[0] != loc.shape[0]:
            raise VxbaError(f"{loc.shape[0]} corner locations for {occ.shape[0]} occupancy words")
        nd = C.c_int64()
        pc = params.as_c() if params is not None else None
        self._check(self._L.vxba_loopsearch_describe(self._h, C.c_int64(loc.shape[0]), _ptr(loc), _ptr(occ),
                                                     C.cast(C.byref(pc), C.c_void_p) if pc is not None else None, C.byref(nd)), "vxba_loopsearch_describe")
        return int(nd.value)

    def read_descriptors(self):
        """dict(triangle (nd, 3), centre (nd, 3), corners (nd, 3) int32: the corner indices of A, B, C) of the current set."""
        nd = self.num_descriptors(-2)
        tri = np.zeros((nd, 3)); ctr = np.zeros((nd, 3)); cor = np.zeros((nd, 3), dtype=np.int32)
        self._check(self._L.vxba_loopsearch_read_descriptors(self._h, _ptr(tri), _ptr(ctr), _ptr(cor)),
                    "vxba_loopsearch_read_descriptors")
        return dict(triangle=tri, centre=ctr, corners=cor)

    def search(self, cloud_cur: int, params: "LoopSearchParams | None" = None):
        """The current set against the database.  Returns dict(frame (-1: none), score, pose (12,), candidates: one dict per verified candidate
        (frame, votes, pairs, hypotheses, best, max_vote, useful, score, pose), launches, host_syncs)."""
        nc = params.candidate_num if params is not None else 20
        frame, ncand, score = C.c_int(-1), C.c_int(0), C.c_double(0.0)
        pose = np.zeros(12); ti = np.zeros((max(nc, 1), self.CAND_INTS), dtype=np.int64); td = np.zeros((max(nc, 1), self.CAND_DOUBLES))
        pc = params.as_c() if params is not None else None
        self._check(self._L.vxba_loopsearch_search(self._h, int(cloud_cur), C.cast(C.byref(pc), C.c_void_p) if pc is not None else None, C.byref(frame), C.byref(score), pose,
                                                   C.byref(ncand), ti, td), "vxba_loopsearch_search")
        names = ("frame", "votes", "pairs", "hypotheses", "best", "max_vote", "useful")
        cands = [dict({k: int(v) for k, v in zip(names, ti[c])}, score=float(td[c, 0]), pose=td[c, 1:].copy()) for c in range(ncand.value)]
        st = self.stats()
        return dict(frame=frame.value, score=score.value, pose=pose, candidates=cands, launches=st["launches"], host_syncs=st["host_syncs"])

    def search_multi(self, dbs, skip_near_num, cloud_cur: int, params: "LoopSearchParams | None" = None):
        """The current set of this handle against the databases of ``dbs`` (``LoopSearch`` handles on the same registration handle; this one may be
        among them) in one search: ``skip_near_num[s]`` replaces ``params.skip_near_num`` for session s, and the query's frame number is this
        handle's ``num_frames()`` in every session.  Returns one dict per session in the form ``search`` returns, each with the call's ``launches``
        and ``host_syncs`` (they do not depend on the number of sessions)."""
        S = len(dbs)
        skips = [int(k) for k in skip_near_num]
        if len(skips) != S:
            raise VxbaError(f"search_multi: VXBA_ERR_ARG: {S} sessions for {len(skips)} skip_near_num")
        nc = max(params.candidate_num if params is not None else 20, 1)
        rows = max(S, 1)
        frame, ncand = (C.c_int * rows)(), (C.c_int * rows)()
        score = np.zeros(rows); pose = np.zeros((rows, 12))
        ti = np.zeros((rows * nc, self.CAND_INTS), dtype=np.int64); td = np.zeros((rows * nc, self.CAND_DOUBLES))
        hs = (C.c_void_p * rows)(*[getattr(d, "_h", None) for d in dbs])
        pc = params.as_c() if params is not None else None
        self._check(self._L.vxba_loopsearch_search_multi(self._h, S, hs, (C.c_int * rows)(*skips), int(cloud_cur), C.cast(C.byref(pc), C.c_void_p) if pc is not None else None,
                                                         frame, score, pose, ncand, ti, td), "vxba_loopsearch_search_multi")
        self._multi_sessions = S
        names = ("frame", "votes", "pairs", "hypotheses", "best", "max_vote", "useful")
        st = self.stats()
        out = []
        for s in range(S):
            cands = [dict({k: int(v) for k, v in zip(names, ti[s * nc + c])}, score=float(td[s * nc + c, 0]), pose=td[s * nc + c, 1:].copy()) for c in range(ncand[s])]
            out.append(dict(frame=int(frame[s]), score=float(score[s]), pose=pose[s].copy(), candidates=cands, launches=st["launches"], host_syncs=st["host_syncs"]))
        return out

    def read_match_offsets(self):
        """Where every session's part of the last ``search_multi``'s match list starts, and the list's length: (S + 1,) int64."""
        out = np.zeros(getattr(self, "_multi_sessions", 0) + 1, dtype=np.int64)
        self._check(self._L.vxba_loopsearch_read_match_offsets(self._h, out), "vxba_loopsearch_read_match_offsets")
        return out

    def read_matches(self):
        """The ordered match list of the last search, (n, 3) int32: (query descriptor, frame, index within the frame).  After ``search_multi``: the
        sessions' lists one after the other (``read_match_offsets``), the frame column counting on from the frames of the sessions before."""
        n = C.c_int64()
        self._check(self._L.vxba_loopsearch_read_matches(self._h, 0, None, C.byref(n)), "vxba_loopsearch_read_matches")
        rows = np.zeros((n.value, 3), dtype=np.int32)
        if n.value:
            self._check(self._L.vxba_loopsearch_read_matches(self._h, n.value, _ptr(rows), C.byref(n)), "vxba_loopsearch_read_matches")
        return rows

    def add(self, cloud_id: int) -> int:
        """The current set becomes the next frame, bound to plane cloud ``cloud_id``; returns the frame number."""
        self._check(self._L.vxba_loopsearch_add(self._h, int(cloud_id)), "vxba_loopsearch_add")
        self.cloud_ids.append(int(cloud_id))
        return self.num_frames() - 1

    def stats(self):
        st = np.zeros(6, dtype=np.int64)
        self._L.vxba_loopsearch_stats(self._h, st)
        return dict(launches=int(st[0]), host_syncs=int(st[1]), frames=int(st[2]), descriptors=int(st[3]), record_bytes=int(st[4]), table_bytes=int(st[5]))


def pack_edges(edges):
    """Edge dicts (i, j, rot, tra, v6) -> (edge_ij (n, 2) int32, edge_data (n, 18)): the records of ``vxba_hba_pass`` (rotation row-major)."""
    n = len(edges)
    ij = np.zeros((n, 2), dtype=np.int32); data = np.zeros((n, 18))
    for k, e in enumerate(edges):
        ij[k] = (e["i"], e["j"])
        data[k, :9] = np.asarray(e["rot"], dtype=np.float64).reshape(9)
        data[k, 9:12] = e["tra"]
        data[k, 12:18] = e["v6"]
    return ij, data


def cov_add_build(xyz_world, var, cell_ptr, device: int = 0):
    """cov_add of OctoTree::push (voxel_map.hpp:91-106, 990-992) per cell: n_cells x 9 x 9."""
    L = load_library()
    cp = np.ascontiguousarray(cell_ptr, dtype=np.int64); n = cp.shape[0] - 1
    xyz = _c(xyz_world).reshape(-1, 3)
    var9 = np.ascontiguousarray(np.transpose(np.asarray(var, dtype=np.float64).reshape(-1, 3, 3), (0, 2, 1)))
    out = np.zeros((n, 81))
    rc = L.vxba_cov_add_build(device, n, xyz.shape[0], xyz, var9, cp, out)
    if rc != 0:
        raise VxbaError(f"vxba_cov_add_build: {_ERRNAMES.get(rc, rc)}")
    return np.transpose(out.reshape(n, 9, 9), (0, 2, 1)).copy()


def plane_update(clusters, eig_val, eig_vec, cov_add, device: int = 0):
    """OctoTree::plane_update (voxel_map.hpp:1118-1146) batched: dict(center, normal, plane_var n x 6 x 6, radius)."""
    L = load_library()
    cl = _c(clusters).reshape(-1, 10); n = cl.shape[0]
    ca = np.ascontiguousarray(np.transpose(np.asarray(cov_add, dtype=np.float64).reshape(n, 9, 9), (0, 2, 1))).reshape(n, 81)
    center = np.zeros((n, 3)); normal = np.zeros((n, 3)); pv = np.zeros((n, 36)); rad = np.zeros(n)
    rc = L.vxba_plane_update(device, n, cl, _c(eig_val).reshape(n, 3), _c(eig_vec).reshape(n, 9), ca, center, normal, pv, rad)
    if rc != 0:
        raise VxbaError(f"vxba_plane_update: {_ERRNAMES.get(rc, rc)}")
    return dict(center=center, normal=normal, plane_var=np.transpose(pv.reshape(n, 6, 6), (0, 2, 1)).copy(), radius=rad)


def rccl_unique_id(librccl_path: str) -> bytes:
    """128-byte ncclUniqueId from the given librccl.so (call on one rank, broadcast to the others)."""
    L = load_library()
    buf = C.create_string_buffer(128)
    rc = L.vxba_rccl_unique_id(librccl_path.encode(), C.cast(buf, C.c_void_p))
    if rc != 0:
        raise VxbaError(f"vxba_rccl_unique_id failed: {_ERRNAMES.get(rc, rc)}")
    return buf.raw


def plane_fit(clusters, device: int = 0):
    """K4: batched eig(cluster.cov()) -> (eig_val (n,3), eig_vec (n,9 col-major))."""
    L = load_library()
    cl = _c(clusters).reshape(-1, 10)
    n = cl.shape[0]
    ev = np.zeros((n, 3)); U = np.zeros((n, 9))
    rc = L.vxba_plane_fit(int(device), n, cl, ev, U)
    if rc != 0:
        raise VxbaError(f"vxba_plane_fit failed: {_ERRNAMES.get(rc, rc)}")
    return ev, U


def plane_fit_judge(clusters, min_point=5, min_eigen_value=0.0025, eigen_ratio_thre=1.0, factor_ratio_max=0.12, device: int = 0):
    """K4 + the reference's plane criteria: (eig_val, eig_vec, flags) with flags bits 1 = N > min_point,
    2 = plane_judge (voxel_map.hpp:1015-1019), 4 = lambda0/lambda1 <= factor_ratio_max (voxel_map.hpp:1314)."""
    L = load_library()
    cl = _c(clusters).reshape(-1, 10)
    n = cl.shape[0]
    ev = np.zeros((n, 3)); U = np.zeros((n, 9)); fl = np.zeros(n, dtype=np.uint8)
    rc = L.vxba_plane_fit_judge(int(device), n, cl, int(min_point), float(min_eigen_value), float(eigen_ratio_thre), float(factor_ratio_max), ev, U, fl)
    if rc != 0:
        raise VxbaError(f"vxba_plane_fit_judge failed: {_ERRNAMES.get(rc, rc)}")
    return ev, U, fl


def build_clusters(xyz, cell_ptr, device: int = 0):
    """Stand-alone K1: packed clusters (n_cells, 10) of bucketed points."""
    L = load_library()
    xyz = _c(xyz).reshape(-1, 3)
    ptr = np.ascontiguousarray(cell_ptr, dtype=np.int64)
    out = np.zeros((ptr.shape[0] - 1, 10))
    rc = L.vxba_build_clusters(int(device), ptr.shape[0] - 1, xyz.shape[0], xyz, ptr, out)
    if rc != 0:
        raise VxbaError(f"vxba_build_clusters failed: {_ERRNAMES.get(rc, rc)}")
    return out


def debug_mfma_probe(A, B, device: int = 0):
    """D = A (16x4) @ B (4x16) through one f64 MFMA with the lane maps K3 assumes."""
    L = load_library()
    D = np.zeros((16, 16))
    rc = L.vxba_debug_mfma_probe(int(device), _c(A).reshape(16, 4), _c(B).reshape(4, 16), D)
    if rc != 0:
        raise VxbaError(f"vxba_debug_mfma_probe failed: {_ERRNAMES.get(rc, rc)}")
    return D


DEBUG_NAN_BITS = 0x7FF8DEB65017E000     # VXBA_DEBUG_NAN_BITS: what vxba_debug_lm_solve leaves in every field of the LM state it does not set


def debug_lm_solve(W: int, Hwork, Jwork, u: float, Rp=None, c: int = 0, done: int = 0, li_rec=None, li_seq: int = 0, want_li_out: bool = True, device: int = 0):
    """The narrow damped solve (1 <= W <= 10) on one system: Hwork (6W, 6W) symmetric gauge-fixed Hessian (stored column-major for the kernel),
    Jwork (6W), poses Rp (W, 12).  li_rec: the LiDAR-inertial record [u | poses 12W | e 6W | E column-major] -> the reduced pose system.
    Returns dict(dxi, xt, q1[, li_out]); with done != 0 every output is the NaN DEBUG_NAN_BITS."""
    L = load_library()
    n = 6 * int(W)
    Hc = np.ascontiguousarray(np.asarray(Hwork, dtype=np.float64).reshape(n, n).T)    # C order of the transpose == column-major of H
    Jc = _c(Jwork).reshape(n)
    rp = None if Rp is None else _c(Rp).reshape(12 * int(W))
    rec = None if li_rec is None else _c(li_rec).reshape(-1)
    if rec is not None and rec.size != 1 + 18 * W + 36 * W * W:
        raise ValueError("li_rec: 1 + 12W + 6W + (6W)^2 doubles")
    dxi, xt, q1 = np.zeros(n), np.zeros(12 * int(W)), C.c_double(0.0)
    lo = np.zeros(18 * int(W) + 1) if (rec is not None and want_li_out) else None
    rc = L.vxba_debug_lm_solve(int(device), int(W), Hc, Jc, float(u), _ptr(rp), int(c), int(done),
                               _ptr(rec), int(li_seq), dxi, xt, C.byref(q1), _ptr(lo))
    if rc != 0:
        raise VxbaError(f"vxba_debug_lm_solve failed: {_ERRNAMES.get(rc, rc)}")
    out = {"dxi": dxi, "xt": xt.reshape(int(W), 12), "q1": np.float64(q1.value)}
    if lo is not None:
        out["li_out"] = lo
    return out


def debug_wide_solve(packed, n: int, u: float, give_up: bool = False, device: int = 0):
    """One step of the wide windows' persistent Cholesky on packed = [H column-major n^2 | JacT n | residual].  Returns dict(info, dxi, q1, residual1);
    info: 0 solved, > 0 non-positive pivot, -1 a device-wide barrier gave up (forced by give_up) -- then the outputs keep their NaN prefill."""
    L = load_library()
    n = int(n)
    pk = _c(packed).reshape(n * n + n + 1)
    dxi, q1, r1, info = np.full(n, np.nan), np.full(1, np.nan), np.full(1, np.nan), C.c_int(0)
    rc = L.vxba_debug_wide_solve(int(device), n, pk, float(u), 1 if give_up else 0, dxi, q1, r1, C.byref(info))
    if rc != 0:
        raise VxbaError(f"vxba_debug_wide_solve failed: {_ERRNAMES.get(rc, rc)}")
    return {"info": int(info.value), "dxi": dxi, "q1": q1[0], "residual1": r1[0]}


def debug_host_damped_step(W: int, Hess, JacT, u: float, Rp):
    """The host's damped step (gauge fix, pivoted LDL^T, trial poses, q1) on one system; Hess (6W, 6W) symmetric, not gauge-fixed.  No GPU needed."""
    L = load_library()
    n = 6 * int(W)
    Hc = np.ascontiguousarray(np.asarray(Hess, dtype=np.float64).reshape(n, n).T)
    xt, dxi, q1 = np.zeros(12 * int(W)), np.zeros(n), C.c_double(0.0)
    rc = L.vxba_debug_host_damped_step(int(W), Hc, _c(JacT).reshape(n), float(u), _c(Rp).reshape(12 * int(W)), xt, dxi, C.byref(q1))
    if rc != 0:
        raise VxbaError(f"vxba_debug_host_damped_step failed: {_ERRNAMES.get(rc, rc)}")
    return {"dxi": dxi, "xt": xt.reshape(int(W), 12), "q1": np.float64(q1.value)}


def debug_stamps(n_waves: int, clear: bool = False):
    """Per-wave s_memtime stamps of the instrumented kernels: array (n_waves, 32) of uint64."""
    L = load_library()
    out = np.zeros((n_waves, 32), dtype=np.uint64)
    L.vxba_debug_stamps(int(clear), _ptr(out), out.size)
    return out


class LocalMap(_Handle):
    """The incremental local map on the GPU (include/vxba.h ``vxba_map_*``; reference: ``surf_map`` / ``surf_map_slide`` of OctoTree nodes,
    voxel_map.hpp:896-1639, driven as voxelslam.cpp:1592-1700 does)."""
    _prefix = "vxba_map"

    def __init__(self, voxel_size=1.0, max_layer=2, min_point=(5, 5, 5, 5), min_eigen_value=0.0025, plane_eigen_value_thre=(0.25, 0.25, 0.25, 0.25),
                 max_points=100, win_size=10, thread_num=5, device=0):
        self.win_size = int(win_size)
        p = MapParams(float(voxel_size), int(max_layer), (C.c_double * 4)(*min_point), float(min_eigen_value), (C.c_double * 4)(*plane_eigen_value_thre),
                      int(max_points), int(win_size), int(thread_num))
        self._create(C.byref(p), int(device))

    def cut_voxel(self, ord_, pnt_body, var_world, pwld):
        pnt = np.ascontiguousarray(pnt_body, dtype=np.float64).reshape(-1, 3)
        var = np.ascontiguousarray(np.transpose(np.asarray(var_world, dtype=np.float64).reshape(-1, 3, 3), (0, 2, 1)))
        self._chk(self._L.vxba_map_cut_voxel(self._h, int(ord_), pnt.shape[0], pnt, var.reshape(-1, 9), np.ascontiguousarray(pwld, dtype=np.float64).reshape(-1, 3)))

    @staticmethod
    def _var9(var, n):
        """n x 3 x 3 (or n x 9 row-major) variances -> the ABI's n x 9 column-major block; None stays None (= all zero)."""
        if var is None:
            return None
        return np.ascontiguousarray(np.transpose(np.asarray(var, dtype=np.float64).reshape(n, 3, 3), (0, 2, 1))).reshape(n, 9)

    def cut_voxel_fix(self, pnt_world, var=None, jour=0.0):
        """World-frame points into the map as FIXED points (``cut_voxel(surf_map, pvec, win_size, jour)``, voxel_map.hpp:1641-1671: what
        keyframe_loading does with a keyframe of an earlier pass).  ``var`` None = zero variances; new roots are stamped with ``jour``."""
        pnt = np.ascontiguousarray(pnt_world, dtype=np.float64).reshape(-1, 3)
        v = self._var9(var, pnt.shape[0])
        self._chk(self._L.vxba_map_cut_voxel_fix(self._h, pnt.shape[0], _ptr(pnt), _ptr(v), float(jour)))

    def cut_voxel_fix_device(self, n, d_pnt_world, d_var=None, jour=0.0):
        """The same on device arrays (raw device addresses, e.g. ``tensor.data_ptr()``; ``d_var`` n x 9 column-major or None)."""
        self._chk(self._L.vxba_map_cut_voxel_fix_device(self._h, int(n), _dev(d_pnt_world), _dev(d_var), float(jour)))

    def clear(self):
        """loop_update's teardown / system_reset: an empty map, ring reset, allocations kept."""
        self._chk(self._L.vxba_map_clear(self._h))

    def set_plane_thresholds(self, min_eigen_value, plane_eigen_value_thre):
        """New plane thresholds for an empty map (the two phases of ``motion_init``); ``VXBA_ERR_STATE`` on a map that holds anything."""
        thre = np.ascontiguousarray(plane_eigen_value_thre, dtype=np.float64).reshape(4)
        self._chk(self._L.vxba_map_set_plane_thresholds(self._h, float(min_eigen_value), thre))

    def loop_update(self, clouds, cloud_vars=None, poses=None, scans=None, est: "LioEstimator | None" = None, jour=0.0):
        """The map's part of loop_update (voxelslam.cpp:1101-1186): clear -> ``clouds`` (a list of n_c x 3 world-frame arrays; ``cloud_vars`` the
        matching list of n_c x 3 x 3 variances, or None) as fixed points in order -> the window's scans under the corrected ``poses`` (win_count x 12)
        -> recut of every root.  ``scans`` None re-cuts the scans resident in the ring slots; otherwise a list of (pnt_body, var_world) per window scan."""
        clouds = [np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds]
        cptr = np.zeros(len(clouds) + 1, dtype=np.int64)
        cptr[1:] = np.cumsum([c.shape[0] for c in clouds])
        pw = np.ascontiguousarray(np.concatenate(clouds)) if clouds else np.zeros((0, 3))
        cv = None
        if cloud_vars is not None:
            cv = np.ascontiguousarray(np.concatenate([self._var9(v, c.shape[0]) for v, c in zip(cloud_vars, clouds)])) if clouds else np.zeros((0, 9))
        Rp = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12) if poses is not None else np.zeros((0, 12))
        win_count = Rp.shape[0]
        sptr = pb = vw = None
        if scans is not None:
            if len(scans) != win_count:
                raise ValueError("loop_update: one (pnt_body, var_world) pair per pose")
            bodies = [np.asarray(s[0], dtype=np.float64).reshape(-1, 3) for s in scans]
            sptr = np.zeros(win_count + 1, dtype=np.int64)
            sptr[1:] = np.cumsum([b.shape[0] for b in bodies])
            pb = np.ascontiguousarray(np.concatenate(bodies)) if bodies else np.zeros((0, 3))
            vw = np.ascontiguousarray(np.concatenate([self._var9(s[1], b.shape[0]) for s, b in zip(scans, bodies)])) if bodies else np.zeros((0, 9))
        self._chk(self._L.vxba_map_loop_update(self._h, len(clouds), _ptr(cptr), _ptr(pw), _ptr(cv), float(jour), win_count, _ptr(Rp), _ptr(sptr), _ptr(pb), _ptr(vw),
                                               est._h if est is not None else None))

    def loop_update_device(self, cloud_ptr, d_pnt_world, d_var=0, poses=None, est: "LioEstimator | None" = None, jour=0.0):
        """``loop_update`` with the clouds in device memory (raw addresses; ``cloud_ptr`` the host offsets, e.g. what ``KeyframeArchive.map_loop``
        returns) and the window's scans re-cut where the ring slots hold them.  Byte-identical to the host route on the same numbers."""
        cptr = np.ascontiguousarray(cloud_ptr, dtype=np.int64).reshape(-1)
        Rp = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 12) if poses is not None else np.zeros((0, 12))
        self._chk(self._L.vxba_map_loop_update_device(self._h, max(cptr.shape[0] - 1, 0), _ptr(cptr), _dev(d_pnt_world), _dev(d_var), float(jour), Rp.shape[0], _ptr(Rp),
                                                      est._h if est is not None else None))

    def scan_device(self, i: int):
        """The resident scan of window position ``i``: dict(n, pnt_body, var_world) with raw device addresses (n x 3 and n x 9 float64), valid until the
        slot is written again -- what ``KeyframeBuilder.push_scan_device`` takes after ``margi``.  ``VXBA_ERR_STATE`` for a slot that holds no scan."""
        n, a, b = C.c_int64(), C.c_void_p(), C.c_void_p()
        self._chk(self._L.vxba_map_scan_device(self._h, int(i), C.byref(n), C.byref(a), C.byref(b)))
        return dict(n=int(n.value), pnt_body=a.value or 0, var_world=b.value or 0)

    def cut_voxel_lio(self, ord_, est: "LioEstimator"):
        """cut_voxel_multi on the scan resident in the odometry handle after ``est.pvec_update(..., resident=True)``."""
        self._chk(self._L.vxba_map_cut_voxel_lio(self._h, int(ord_), est._h))

    def export_planes(self, est: "LioEstimator") -> int:
        """Plane records of the changed part of the tree into the odometry's plane map, on the device."""
        n = C.c_int64(0)
        self._chk(self._L.vxba_map_export_planes(self._h, est._h, C.byref(n)))
        return int(n.value)

    def recut(self, win_count, poses, factor: "LidarFactor"):
        n = C.c_int64(0)
        self._chk(self._L.vxba_map_recut(self._h, int(win_count), np.ascontiguousarray(poses, dtype=np.float64)[:win_count], factor._h, C.byref(n)))
        return int(n.value)

    def margi(self, win_count, poses, factor: "LidarFactor"):
        self._chk(self._L.vxba_map_margi(self._h, int(win_count), np.ascontiguousarray(poses, dtype=np.float64)[:win_count], factor._h))

    def slide(self, mgsize=1):
        self._chk(self._L.vxba_map_slide(self._h, int(mgsize)))

    def counts(self):
        out = np.zeros(4, dtype=np.int64)
        self._chk(self._L.vxba_map_counts(self._h, out))
        return dict(roots=int(out[0]), slide=int(out[1]), leaves=int(out[2]), mp0=int(out[3]))

    def fix_pool(self):
        """Pool of the marginalised points: cursor / capacity in points, compactions so far (include/vxba.h ``vxba_map_fix_pool``)."""
        out = np.zeros(3, dtype=np.int64)
        self._chk(self._L.vxba_map_fix_pool(self._h, out))
        return dict(cursor=int(out[0]), capacity=int(out[1]), compactions=int(out[2]))

    def set_journey(self, jour: float):
        """The journey odometer the next margi stamps on the slide map's roots (voxelslam.cpp:1349, 1677)."""
        self._chk(self._L.vxba_map_set_journey(self._h, float(jour)))

    def release(self, jour_now: float, min_age: int = 700, est: "LioEstimator | None" = None):
        """The release branch of the local-mapping loop (voxelslam.cpp:1503-1523): roots last seen ``min_age`` journeys ago leave the map,
        the node pool is compacted.  Returns dict(roots, nodes) released."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.vxba_map_release(self._h, float(jour_now), int(min_age), est._h if est is not None else None, C.byref(a), C.byref(b)))
        return dict(roots=int(a.value), nodes=int(b.value))

    def device_bytes(self):
        out = np.zeros(5, dtype=np.int64)
        self._chk(self._L.vxba_map_device_bytes(self._h, out))
        return dict(nodes=int(out[0]), fix_pool=int(out[1]), scans=int(out[2]), other=int(out[3]), total=int(out[4]))

    def leaves(self):
        """Every leaf, sorted by node id, as a dictionary of arrays (fields of include/vxba.h ``vxba_map_leaves``)."""
        W = self.win_size
        n = C.c_int64(0)
        self._chk(self._L.vxba_map_leaves(self._h, 0, None, None, None, C.byref(n)))
        n = int(n.value)
        ids = np.zeros(n, dtype=np.uint64); ints = np.zeros((n, 8), dtype=np.int32); d = np.zeros((n, 156 + 11 * W))
        got = C.c_int64(0)
        if n:
            self._chk(self._L.vxba_map_leaves(self._h, n, _ptr(ids), _ptr(ints), _ptr(d), C.byref(got)))
            assert got.value == n
        o = np.argsort(ids, kind="stable")
        ids, ints, d = ids[o], ints[o], d[o]
        return dict(node_id=ids, layer=ints[:, 0], isexist=ints[:, 1].astype(bool), is_plane=ints[:, 2].astype(bool), has_sw=ints[:, 3].astype(bool),
                    opt_state=ints[:, 4], last_num=ints[:, 5], n_point_fix=ints[:, 6], in_slide=ints[:, 7].astype(bool),
                    pcr_add=d[:, 0:10], pcr_fix=d[:, 10:20], eig_val=d[:, 20:23], eig_vec=d[:, 23:32], center=d[:, 32:35], normal=d[:, 35:38],
                    radius=d[:, 38], plane_var=np.transpose(d[:, 39:75].reshape(n, 6, 6), (0, 2, 1)), cov_add=np.transpose(d[:, 75:156].reshape(n, 9, 9), (0, 2, 1)),
                    pcrs_local=d[:, 156:156 + 10 * W].reshape(n, W, 10), n_points=d[:, 156 + 10 * W:].astype(np.int64))

    def leaf_points(self, node_id, which):
        """Points a leaf keeps for a later subdivision (``vxba_map_leaf_points``): which = -1 the fix points (world, pool order), which = i the
        window's i-th scan (body, the order of the leaf's range): (n, 3), (n, 3, 3).  ``VxbaError`` when no leaf has the id."""
        n = C.c_int64(0)
        self._chk(self._L.vxba_map_leaf_points(self._h, int(node_id), int(which), 0, None, C.byref(n)))
        n = int(n.value)
        buf = np.zeros((n, 12))
        if n:
            got = C.c_int64(0)
            self._chk(self._L.vxba_map_leaf_points(self._h, int(node_id), int(which), n, _ptr(buf), C.byref(got)))
            assert got.value == n
        return buf[:, :3].copy(), np.transpose(buf[:, 3:].reshape(n, 3, 3), (0, 2, 1)).copy()


class KeyframeParams(C.Structure):
    """``vxba_keyframe_params``; a value <= 0 means the reference's (10 scans, voxel_size 1.0 -- the filter runs at a tenth of it --, 5 deg, 0.1 m)."""
    _fields_ = [("win_size", C.c_int), ("voxel_size", C.c_double), ("ang_deg", C.c_double), ("len", C.c_double)]


class KeyframeBuilder(_Handle):
    """``vxba_keyframe_*``: marginalised scans in, keyframes out (the front half of thd_loop_closure, voxelslam.cpp:1898-1977, and down_sampling_pvec).
    The buffered scans and the keyframe's two clouds stay on the device: ``full`` (N, 3) float32 for the loop chain, ``down`` (n_down, 6) float32
    (x, y, z, var00, var11, var22) for the hierarchical BA.  See include/vxba.h for the rule and the arithmetic that is pinned bit for bit."""

    _prefix = "vxba_keyframe"

    def __init__(self, win_size: int = 10, voxel_size: float = 1.0, ang_deg: float = 5.0, len_thr: float = 0.1, device: int = 0):
        prm = KeyframeParams(int(win_size), float(voxel_size), float(ang_deg), float(len_thr))
        self._create(int(device), C.byref(prm))

    def clear(self):
        self._check(self._L.vxba_keyframe_clear(self._h), "vxba_keyframe_clear")

    def push_scan(self, pose, v6, pnt_body, var=None) -> bool:
        """One ScanPose: pose (12,), v6 (6,), body points (n, 3), covariances (n, 3, 3) or (n, 9) column-major (symmetric: either order) or None = zeros.
        True when the push made a keyframe."""
        p = _c(pnt_body).reshape(-1, 3)
        v = None if var is None else _c(var).reshape(-1, 9)
        if v is not None and v.shape[0] != p.shape[0]:
            raise ValueError("one covariance per point")
        em = C.c_int()
        self._check(self._L.vxba_keyframe_push_scan(self._h, _c(pose).reshape(12), _c(v6).reshape(6), C.c_int64(p.shape[0]), _ptr(p),
                                                    _ptr(v), C.byref(em)), "vxba_keyframe_push_scan")
        return bool(em.value)

    def push_scan_device(self, pose, v6, n: int, d_pnt_body: int, d_var: int = 0) -> bool:
        """The same with the points (n, 3) and covariances (n, 9; 0 = zeros) in device memory (raw addresses, float64)."""
        em = C.c_int()
        self._check(self._L.vxba_keyframe_push_scan_device(self._h, _c(pose).reshape(12), _c(v6).reshape(6), C.c_int64(int(n)), _dev(d_pnt_body),
                                                           _dev(d_var), C.byref(em)), "vxba_keyframe_push_scan_device")
        return bool(em.value)

    def info(self):
        """The last keyframe: dict(id, pose, jour, n_full, n_down), or None before the first."""
        kid, nf, nd, jour = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        pose = np.zeros(12)
        rc = self._L.vxba_keyframe_info(self._h, C.byref(kid), pose, C.byref(jour), C.byref(nf), C.byref(nd))
        if rc == 4:
            return None
        self._check(rc, "vxba_keyframe_info")
        return dict(id=int(kid.value), pose=pose, jour=float(jour.value), n_full=int(nf.value), n_down=int(nd.value))

    def read(self):
        """(full (N, 3) float32, down (n_down, 6) float32) of the last keyframe."""
        i = self.info()
        if i is None:
            raise VxbaError("vxba_keyframe_read: VXBA_ERR_STATE: no keyframe yet")
        full = np.zeros((i["n_full"], 3), dtype=np.float32); down = np.zeros((i["n_down"], 6), dtype=np.float32)
        self._check(self._L.vxba_keyframe_read(self._h, _ptr(full), _ptr(down)), "vxba_keyframe_read")
        return full, down

    def device_ptrs(self):
        """Raw device addresses of the last keyframe's clouds (0 for an empty one), valid until the next emitting push: dict(full, down, down_xyz) --
        down_xyz is the (n_down, 3) packed copy of down's first three columns."""
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._L.vxba_keyframe_device(self._h, C.byref(a), C.byref(b)), "vxba_keyframe_device")
        self._check(self._L.vxba_keyframe_device_down_xyz(self._h, C.byref(c)), "vxba_keyframe_device_down_xyz")
        return dict(full=a.value or 0, down=b.value or 0, down_xyz=c.value or 0)

    def num_scans(self) -> int:
        return int(self._L.vxba_keyframe_num_scans(self._h))

    def num_buffered(self) -> int:
        return int(self._L.vxba_keyframe_num_buffered(self._h))

    def scan_poses(self, first: int = 0, count: "int | None" = None):
        """(poses (count, 12), v6 (count, 6)) of the ScanPoses pushed since clear."""
        if count is None:
            count = self.num_scans() - first
        P = np.zeros((max(count, 0), 12)); V = np.zeros((max(count, 0), 6))
        self._check(self._L.vxba_keyframe_scan_poses(self._h, C.c_int64(first), C.c_int64(count), P.reshape(-1) if P.size else np.zeros(1), V.reshape(-1) if V.size else np.zeros(1)),
                    "vxba_keyframe_scan_poses")
        return P, V

    def stats(self):
        st = np.zeros(4, dtype=np.int64)
        self._L.vxba_keyframe_stats(self._h, st)
        return dict(launches=int(st[0]), host_waits=int(st[1]), bytes_d2h=int(st[2]), bytes_h2d=int(st[3]))

    def set_profiling(self, enable: bool = True):
        self._check(self._L.vxba_keyframe_set_profiling(self._h, 1 if enable else 0), "vxba_keyframe_set_profiling")

    def stage_times(self):
        """[ms] of the last (profiled) emitting push: dict(assembly, sort_group, filter), from events between the stages."""
        ms = np.zeros(3)
        self._check(self._L.vxba_keyframe_stage_times(self._h, ms), "vxba_keyframe_stage_times")
        return dict(assembly=float(ms[0]), sort_group=float(ms[1]), filter=float(ms[2]))


class KeyframeArchive(_Handle):
    """``vxba_kfarchive_*``: the running session's keyframes on the device (``down`` clouds (n, 6) float32, ids, poses x0, journeys, exist flags) and
    what brings them back into the local map: ``map_loop`` (voxelslam.cpp:2131-2150), ``load_near`` (keyframe_loading, :1189-1228).  World points
    and variances come out as raw device addresses for ``LocalMap.loop_update_device`` / ``cut_voxel_fix_device``.  See include/vxba.h for the quirks kept."""

    _prefix = "vxba_kfarchive"

    def __init__(self, device: int = 0):
        self._create(int(device))

    def clear(self):
        self._check(self._L.vxba_kfarchive_clear(self._h), "vxba_kfarchive_clear")

    def add(self, kf_id: int, pose, jour: float, down_xyzv):
        d = np.ascontiguousarray(down_xyzv, dtype=np.float32).reshape(-1, 6)
        self._check(self._L.vxba_kfarchive_add(self._h, int(kf_id), _c(pose).reshape(12), float(jour), d.shape[0], _ptr(d)), "vxba_kfarchive_add")

    def add_device(self, kf_id: int, pose, jour: float, n: int, d_down_xyzv: int):
        """The same with the (n, 6) float32 cloud in device memory (a raw address, e.g. ``KeyframeBuilder.device_ptrs()["down"]``)."""
        self._check(self._L.vxba_kfarchive_add_device(self._h, int(kf_id), _c(pose).reshape(12), float(jour), int(n), _dev(d_down_xyzv)), "vxba_kfarchive_add_device")

    def add_from(self, builder: "KeyframeBuilder"):
        """The builder's last keyframe, device to device."""
        i = builder.info()
        if i is None:
            raise VxbaError("KeyframeArchive.add_from: VXBA_ERR_STATE: the builder holds no keyframe")
        self.add_device(i["id"], i["pose"], i["jour"], i["n_down"], builder.device_ptrs()["down"])

    def __len__(self) -> int:
        return int(self._L.vxba_kfarchive_num(self._h))

    def info(self, k: int):
        kid, n, ex, jour = C.c_int64(), C.c_int64(), C.c_int(), C.c_double()
        pose = np.zeros(12)
        self._check(self._L.vxba_kfarchive_info(self._h, int(k), C.byref(kid), pose, C.byref(jour), C.byref(n), C.byref(ex)), "vxba_kfarchive_info")
        return dict(id=int(kid.value), pose=pose, jour=float(jour.value), n=int(n.value), exist=int(ex.value))

    def ids(self):
        return np.array([self.info(k)["id"] for k in range(len(self))], dtype=np.int64)

    def exist(self):
        return np.array([self.info(k)["exist"] for k in range(len(self))], dtype=np.int32)

    def read(self, k: int):
        out = np.zeros((self.info(k)["n"], 6), dtype=np.float32)
        self._check(self._L.vxba_kfarchive_read(self._h, int(k), _ptr(out)), "vxba_kfarchive_read")
        return out

    def device_ptrs(self):
        """dict(xyzv: raw device address of the packed store (0 when empty), cloud_ptr: a copy of the K + 1 host offsets)."""
        a, b = C.c_void_p(), C.c_void_p()
        self._check(self._L.vxba_kfarchive_device(self._h, C.byref(a), C.byref(b)), "vxba_kfarchive_device")
        K = len(self)
        return dict(xyzv=a.value or 0, cloud_ptr=np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_int64)), shape=(K + 1,)).copy())

    def set_poses(self, x0):
        x = _c(x0).reshape(-1, 12)
        if x.shape[0] != len(self):
            raise ValueError("set_poses: one pose per keyframe")
        self._check(self._L.vxba_kfarchive_set_poses(self._h, _ptr(x)), "vxba_kfarchive_set_poses")

    def arm_history(self, init_num: int = 5):
        self._check(self._L.vxba_kfarchive_arm_history(self._h, int(init_num)), "vxba_kfarchive_arm_history")

    def history_size(self) -> int:
        return int(self._L.vxba_kfarchive_history_size(self._h))

    def load_near(self, p_curr, radius: float = 10.0):
        """keyframe_loading's search and transform: dict(k (-1: nothing loaded), n, pnt_world (raw device address, n x 3 float64))."""
        k, n, a = C.c_int(), C.c_int64(), C.c_void_p()
        self._check(self._L.vxba_kfarchive_load_near(self._h, _c(p_curr).reshape(3), float(radius), C.byref(k), C.byref(n), C.byref(a)), "vxba_kfarchive_load_near")
        return dict(k=int(k.value), n=int(n.value), pnt_world=a.value or 0)

    def map_loop(self, init_num: int = 5, cumulative: bool = True, pending=()):
        """The map_loop build: dict(cloud_ptr (n_clouds + 1,), pnt_world, var) with raw device addresses (x 3 and x 9 float64).  ``pending``: loop_update's
        buffered scans as (pose (12,), n, d_pnt_body, d_var) tuples, appended as further clouds in the same launch.  ``cumulative`` True is upstream as written."""
        init = int(init_num) if init_num > 0 else 5
        P = len(pending)
        cptr = np.zeros(init + P + 1, dtype=np.int64)
        nc, a, b = C.c_int(), C.c_void_p(), C.c_void_p()
        if P == 0:
            rc = self._L.vxba_kfarchive_map_loop(self._h, init, 1 if cumulative else 0, cptr, C.byref(nc), C.byref(a), C.byref(b))
        else:
            poses = np.ascontiguousarray([_c(s[0]).reshape(12) for s in pending])
            ns = np.array([int(s[1]) for s in pending], dtype=np.int64)
            dp = (C.c_void_p * P)(*[int(s[2]) or None for s in pending])
            dv = (C.c_void_p * P)(*[int(s[3]) or None for s in pending])
            rc = self._L.vxba_kfarchive_map_loop_scans(self._h, init, 1 if cumulative else 0, P, _ptr(poses), _ptr(ns), C.cast(dp, C.c_void_p), C.cast(dv, C.c_void_p), cptr,
                                                       C.byref(nc), C.byref(a), C.byref(b))
        self._check(rc, "vxba_kfarchive_map_loop")
        return dict(cloud_ptr=cptr[:nc.value + 1].copy(), pnt_world=a.value or 0, var=b.value or 0)

    def stats(self):
        st = np.zeros(4, dtype=np.int64)
        self._L.vxba_kfarchive_stats(self._h, st)
        return dict(launches=int(st[0]), host_waits=int(st[1]), bytes_d2h=int(st[2]), bytes_h2d=int(st[3]))


@dataclasses.dataclass
class CornerParams:
    """``vxba_corner_params`` (include/vxba.h); the defaults are read_parameters' normal preset (BTC.cpp:7-20, 25), ``CornerParams.preset(True)`` the
    high-fly one (:39-52, 57).  No value inside means "default"."""
    useful_corner_num: int = 100
    plane_merge_normal_thre: float = 0.1
    plane_merge_dis_thre: float = 0.3
    plane_detection_thre: float = 0.01
    voxel_size: float = 1.0
    voxel_init_num: int = 10
    proj_plane_num: int = 2
    proj_image_resolution: float = 0.5
    proj_image_high_inc: float = 0.1
    proj_dis_min: float = 0.0
    proj_dis_max: float = 5.0
    summary_min_thre: float = 10.0
    line_filter_enable: int = 1
    touch_filter_enable: int = 0
    non_max_suppression_radius: float = 2.0

    class _C(C.Structure):
        _fields_ = [("useful_corner_num", C.c_int), ("plane_merge_normal_thre", C.c_double), ("plane_merge_dis_thre", C.c_double), ("plane_detection_thre", C.c_double),
                    ("voxel_size", C.c_double), ("voxel_init_num", C.c_int), ("proj_plane_num", C.c_int), ("proj_image_resolution", C.c_double),
                    ("proj_image_high_inc", C.c_double), ("proj_dis_min", C.c_double), ("proj_dis_max", C.c_double), ("summary_min_thre", C.c_double),
                    ("line_filter_enable", C.c_int), ("touch_filter_enable", C.c_int), ("non_max_suppression_radius", C.c_double)]

    def as_c(self):
        return self._C(*[getattr(self, f.name) for f in dataclasses.fields(self)])

    @classmethod
    def preset(cls, is_high_fly: bool = False):
        """What ``vxba_corner_default_params`` fills in."""
        c = cls._C()
        load_library().vxba_corner_default_params(C.cast(C.byref(c), C.c_void_p), 1 if is_high_fly else 0)
        return cls(*[getattr(c, f.name) for f in dataclasses.fields(cls)])


CORNER_REC = 16


def _plane_records(rec):
    return dict(records=rec, center=rec[:, 0:3], cov=rec[:, 3:9], n_points=rec[:, 9].astype(np.int64), normal=rec[:, 10:13], d=rec[:, 13], radius=rec[:, 14], lambda_min=rec[:, 15])


class CornerExtractor(_Handle):
    """``vxba_corner_*``: a keyframe's cloud in, the corner set ``LoopSearch.describe`` takes out (GenerateSTDescs without generate_std: plane voxels,
    projection planes, projection images, suppression, cut).  See include/vxba.h for the arithmetic that is pinned and the choices it fixes."""

    _prefix = "vxba_corner"
    CAND_INTS = 6
    STAGES = ("planes", "pairs", "pairs_merged", "project", "sort_group", "cells_suppress")

    def __init__(self, device: int = 0):
        self._n_corners = 0                    # of the last extract that succeeded
        self._create(int(device))

    @staticmethod
    def _prm(params):
        pc = params.as_c() if params is not None else None
        return pc, (C.cast(C.byref(pc), C.c_void_p) if pc is not None else None)

    def extract(self, xyz, params: "CornerParams | None" = None) -> int:
        """The corners of a cloud (n, 3) float64 on the host; returns their count (``read`` for the set)."""
        a = _c(xyz).reshape(-1, 3)
        pc, pp = self._prm(params)
        nc = C.c_int64()
        self._check(self._L.vxba_corner_extract(self._h, C.c_int64(a.shape[0]), _ptr(a), pp, C.byref(nc)), "vxba_corner_extract")
        self._n_corners = int(nc.value)
        return self._n_corners

    def extract_device(self, n_points: int, d_xyz: int, params: "CornerParams | None" = None) -> int:
        """The same from (n, 3) float32 in device memory (a raw address: ``KeyframeBuilder.device_ptrs()['full']``), widened exactly."""
        pc, pp = self._prm(params)
        nc = C.c_int64()
        self._check(self._L.vxba_corner_extract_device(self._h, C.c_int64(int(n_points)), _dev(d_xyz), pp, C.byref(nc)), "vxba_corner_extract_device")
        self._n_corners = int(nc.value)
        return self._n_corners

    def extract_with_planes(self, xyz, centres, normals, params: "CornerParams | None" = None) -> int:
        """Stages 4-7 (gate, images, suppression, cut) on a caller's plane list: centres (m, 3), normals (m, 3), used as they are."""
        a = _c(xyz).reshape(-1, 3); c = _c(centres).reshape(-1, 3); nrm = _c(normals).reshape(-1, 3)
        if c.shape != nrm.shape:
            raise ValueError("one normal per centre")
        pc, pp = self._prm(params)
        nc = C.c_int64()
        self._check(self._L.vxba_corner_extract_with_planes(self._h, C.c_int64(a.shape[0]), _ptr(a), C.c_int64(c.shape[0]), _ptr(c),
                                                            _ptr(nrm), pp, C.byref(nc)), "vxba_corner_extract_with_planes")
        self._n_corners = int(nc.value)
        return self._n_corners

    def read(self):
        """dict(locations (n, 3), occupancy (n,) uint64, summary (n,) int32) of the last extract."""
        loc = np.zeros((self._n_corners, 3)); occ = np.zeros(self._n_corners, dtype=np.uint64); sm = np.zeros(self._n_corners, dtype=np.int32)
        self._check(self._L.vxba_corner_read(self._h, _ptr(loc), _ptr(occ), _ptr(sm)), "vxba_corner_read")
        return dict(locations=loc, occupancy=occ, summary=sm)

    def planes(self):
        """Stage 1-2: dict(records (P, 16), center, cov, n_points, normal, d, radius, lambda_min, labels (P,) int32)."""
        n = C.c_int64()
        self._check(self._L.vxba_corner_planes(self._h, C.byref(n), None, None), "vxba_corner_planes")
        rec = np.zeros((n.value, CORNER_REC)); lab = np.zeros(n.value, dtype=np.int32)
        self._check(self._L.vxba_corner_planes(self._h, C.byref(n), _ptr(rec), _ptr(lab)), "vxba_corner_planes")
        return dict(_plane_records(rec), labels=lab)

    def projection_planes(self):
        """Stage 3-4: the final sorted list as ``planes`` gives records, and ``used`` (m,) int32: the position among the used planes or -1."""
        n = C.c_int64()
        self._check(self._L.vxba_corner_projection_planes(self._h, C.byref(n), None, None), "vxba_corner_projection_planes")
        rec = np.zeros((n.value, CORNER_REC)); used = np.zeros(n.value, dtype=np.int32)
        self._check(self._L.vxba_corner_projection_planes(self._h, C.byref(n), _ptr(rec), _ptr(used)), "vxba_corner_projection_planes")
        return dict(_plane_records(rec), used=used)

    def candidates(self):
        """Stage 5-6: per candidate plane, cell_x, cell_y, count, summary, kept (the suppression's verdict), occupancy, location; n_corners: how many
        the cut leaves."""
        n = C.c_int64()
        self._check(self._L.vxba_corner_candidates(self._h, C.byref(n), None, None, None), "vxba_corner_candidates")
        ints = np.zeros((n.value, self.CAND_INTS), dtype=np.int32); occ = np.zeros(n.value, dtype=np.uint64); loc = np.zeros((n.value, 3))
        self._check(self._L.vxba_corner_candidates(self._h, C.byref(n), _ptr(ints), _ptr(occ), _ptr(loc)),
                    "vxba_corner_candidates")
        return dict(plane=ints[:, 0], cell_x=ints[:, 1], cell_y=ints[:, 2], count=ints[:, 3], summary=ints[:, 4], kept=ints[:, 5].astype(bool), occupancy=occ, locations=loc,
                    n_corners=self._n_corners)

    def stats(self):
        st = np.zeros(6, dtype=np.int64)
        self._L.vxba_corner_stats(self._h, st)
        return dict(launches=int(st[0]), host_waits=int(st[1]), bytes_d2h=int(st[2]), bytes_h2d=int(st[3]), cells=int(st[4]), candidates=int(st[5]))

    def set_profiling(self, enable: bool = True):
        self._check(self._L.vxba_corner_set_profiling(self._h, 1 if enable else 0), "vxba_corner_set_profiling")

    def stage_times(self):
        """[ms] per stage (``STAGES``) of the last profiled ``extract`` / ``extract_device``, from events around the stages."""
        ms = np.zeros(len(self.STAGES))
        self._check(self._L.vxba_corner_stage_times(self._h, ms), "vxba_corner_stage_times")
        return dict(zip(self.STAGES, (float(v) for v in ms)))


class SavedSession(_Handle):
    """``vxba_session_*``: the saved scans of an earlier run (``sessionio.read_session``) resident on the device; keyframes, descriptor clouds and the
    set ``global_map`` takes out (the per-point half of previous_map_read, voxelslam.cpp:307-448).  See include/vxba.h for what is kept of upstream."""

    _prefix = "vxba_session"

    def __init__(self, device: int = 0):
        self._create(int(device))

    def clear(self):
        self._check(self._L.vxba_session_clear(self._h), "vxba_session_clear")

    def load_scans(self, scans, poses, scan_ptr=None):
        """``scans``: a list of (n_i, 3) clouds, or -- with ``scan_ptr`` (n + 1 offsets) -- the packed (N, 3) points; ``poses`` (n, 12)."""
        if scan_ptr is None:
            ptr = np.concatenate([[0], np.cumsum([np.asarray(s).reshape(-1, 3).shape[0] for s in scans])]).astype(np.int64)
            parts = [np.asarray(s, dtype=np.float32).reshape(-1, 3) for s in scans]
            xyz = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 3), np.float32)
        else:
            ptr = np.ascontiguousarray(scan_ptr, dtype=np.int64).reshape(-1)
            xyz = np.ascontiguousarray(scans, dtype=np.float32).reshape(-1, 3)
            if ptr.size and ptr.max() > xyz.shape[0]:
                raise ValueError("scan_ptr runs past the points")
        P = _c(poses).reshape(-1, 12)
        if P.shape[0] != ptr.size - 1:
            raise ValueError("one pose per scan")
        self._check(self._L.vxba_session_load_scans(self._h, C.c_int64(ptr.size - 1), ptr, _ptr(xyz), _ptr(P)), "vxba_session_load_scans")

    def num_scans(self) -> int:
        return int(self._L.vxba_session_num_scans(self._h))

    def num_keyframes(self) -> int:
        return int(self._L.vxba_session_num_keyframes(self._h))

    def build_keyframes(self, win_size: int = 10, voxel_size: float = 1.0) -> int:
        k = C.c_int64()
        self._check(self._L.vxba_session_build_keyframes(self._h, int(win_size), float(voxel_size), C.byref(k)), "vxba_session_build_keyframes")
        return int(k.value)

    def keyframes(self):
        """dict(kf_ptr (K + 1,), ids (K,) int64, poses (K, 12): x0)."""
        K = self.num_keyframes()
        ptr = np.zeros(K + 1, dtype=np.int64); ids = np.zeros(K, dtype=np.int64); x0 = np.zeros((K, 12))
        self._check(self._L.vxba_session_keyframes(self._h, _ptr(ptr), _ptr(ids), _ptr(x0)), "vxba_session_keyframes")
        return dict(kf_ptr=ptr, ids=ids, poses=x0)

    def read_keyframes(self):
        """The keyframe clouds: a list of K (n_k, 3) float32 arrays."""
        ptr = self.keyframes()["kf_ptr"]
        xyz = np.zeros((int(ptr[-1]), 3), dtype=np.float32)
        self._check(self._L.vxba_session_read_keyframes(self._h, _ptr(xyz)), "vxba_session_read_keyframes")
        return [xyz[ptr[k]:ptr[k + 1]] for k in range(ptr.size - 1)]

    def device_ptr(self) -> int:
        """Raw device address of the packed clouds (0: no point): with ``keyframes()['kf_ptr']`` what ``HbaSession.add_keyframes_device`` takes."""
        d = C.c_void_p()
        self._check(self._L.vxba_session_device(self._h, C.byref(d)), "vxba_session_device")
        return d.value or 0

    def set_scan_poses(self, poses):
        P = _c(poses).reshape(-1, 12)
        if P.shape[0] != self.num_scans():
            raise ValueError("one pose per scan")
        self._check(self._L.vxba_session_set_scan_poses(self._h, _ptr(P)), "vxba_session_set_scan_poses")

    @staticmethod
    def num_windows(K: int, acsize: int = 10, mgsize: int = 5) -> int:
        return int(load_library().vxba_session_num_windows(C.c_int64(int(K)), int(acsize), int(mgsize)))

    def window_cloud(self, w: int, acsize: int = 10, mgsize: int = 5):
        """dict(n, d_xyz: raw device address valid until the next call, frame_id)."""
        n, d, fid = C.c_int64(), C.c_void_p(), C.c_int64()
        self._check(self._L.vxba_session_window_cloud(self._h, int(w), int(acsize), int(mgsize), C.byref(n), C.byref(d), C.byref(fid)), "vxba_session_window_cloud")
        self._n_win = int(n.value)
        return dict(n=int(n.value), d_xyz=d.value or 0, frame_id=int(fid.value))

    def read_window(self):
        xyz = np.zeros((getattr(self, "_n_win", 0), 3), dtype=np.float32)
        self._check(self._L.vxba_session_read_window(self._h, _ptr(xyz)), "vxba_session_read_window")
        return xyz

    def map_set(self, session_id):
        """This session's keyframes as a set of ``global_map``."""
        k = self.keyframes()
        return dict(d_xyz=self.device_ptr(), cloud_ptr=k["kf_ptr"], poses=k["poses"], id=session_id)

    def stats(self):
        st = np.zeros(4, dtype=np.int64)
        self._L.vxba_session_stats(self._h, st)
        return dict(launches=int(st[0]), host_waits=int(st[1]), points=int(st[2]), keyframes=int(st[3]))

    def set_profiling(self, enable: bool = True):
        self._check(self._L.vxba_session_set_profiling(self._h, 1 if enable else 0), "vxba_session_set_profiling")

    def stage_times(self):
        """[ms] of the last (profiled) ``build_keyframes``: dict(merge, sort_group, mean), from events between the stages."""
        ms = np.zeros(3)
        self._check(self._L.vxba_session_stage_times(self._h, ms), "vxba_session_stage_times")
        return dict(merge=float(ms[0]), sort_group=float(ms[1]), mean=float(ms[2]))


def _globalmap_call(sets, interval_size, out, capacity, device=0):
    """``vxba_globalmap`` as it is: (rc, n_out, chunk_ptr)."""
    L = load_library()
    S = len(sets)
    ptrs = [np.ascontiguousarray(s["cloud_ptr"], dtype=np.int64).reshape(-1) for s in sets]
    poses = [_c(s["poses"]).reshape(-1, 12) for s in sets]
    nk = np.array([p.size - 1 for p in ptrs] + [0], dtype=np.int64)
    for p, q in zip(ptrs, poses):
        if q.shape[0] != p.size - 1:
            raise ValueError("one pose per keyframe")
    a_xyz = (C.c_void_p * max(S, 1))(*[int(s["d_xyz"]) if s["d_xyz"] else None for s in sets])
    a_ptr = (C.c_void_p * max(S, 1))(*[p.ctypes.data for p in ptrs])
    a_pose = (C.c_void_p * max(S, 1))(*[q.ctypes.data if q.size else None for q in poses])
    inten = np.array([float(s["id"]) for s in sets] + [0.0], dtype=np.float32)
    chunks = np.zeros(int(nk.sum()) + 2, dtype=np.int64)
    n_out, n_chunks = C.c_int64(), C.c_int64()
    rc = L.vxba_globalmap(int(device), S, a_xyz, a_ptr, nk, a_pose, inten, C.c_int64(int(interval_size)), _ptr(out), C.c_int64(int(capacity)), C.byref(n_out),
                          _ptr(chunks), C.byref(n_chunks))
    return rc, int(n_out.value), chunks[:int(n_chunks.value) + 1].copy()


def global_map(sets, interval_size: int = 5000000, device: int = 0):
    """``pub_globalmap`` (voxelslam.cpp:108-150) over ``sets`` -- each dict(d_xyz: raw device address of packed float32 clouds, cloud_ptr (K + 1,),
    poses (K, 12), id) as ``SavedSession.map_set`` gives -- in one launch: dict(xyzi (n, 4) float32, chunk_ptr: the bounds of upstream's publishes)."""
    rc, n, _ = _globalmap_call(sets, interval_size, None, 0, device)
    if rc != 0 and n == 0:
        raise VxbaError(f"vxba_globalmap: {_ERRNAMES.get(rc, rc)}")
    out = np.zeros((n, 4), dtype=np.float32)
    rc, n, chunks = _globalmap_call(sets, interval_size, out, n, device)
    if rc != 0:
        raise VxbaError(f"vxba_globalmap: {_ERRNAMES.get(rc, rc)}")
    return dict(xyzi=out, chunk_ptr=chunks)
