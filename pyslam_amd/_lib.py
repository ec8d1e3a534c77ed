"""ctypes binding of libpyslam_hipvol.so (include/hipvol.h).

There is no CPU fallback: if the shared object is missing it is built with hipcc; if that fails, or
no gfx950 device is usable when a volume is created, the call raises.
"""
import ctypes
import os

import numpy as np

from . import build as _build

_c = ctypes
_vp, _i64, _i32, _f32, _f64 = _c.c_void_p, _c.c_int64, _c.c_int32, _c.c_float, _c.c_double
_pi64 = _c.POINTER(_c.c_int64)
_pi32 = _c.POINTER(_c.c_int32)

HV_OK = 0
HV_MODE_VOXEL_GRID = 0
HV_MODE_VOXEL_SEMANTIC_GRID = 1
HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID = 2
HV_MODE_TSDF = 3
HV_MODE_VOXEL_SEMANTIC_GRID2 = 11
HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID2 = 12
HV_HOST, HV_DEVICE = 0, 1
HV_COLOR_NONE, HV_COLOR_U8, HV_COLOR_F32 = 0, 1, 2
HV_DEPTH_F32, HV_DEPTH_U16 = 0, 1


class HvConfig(_c.Structure):
    _fields_ = [
        ("mode", _i32),
        ("device", _i32),
        ("voxel_size", _f64),
        ("sdf_trunc", _f64),
        ("block_size", _i32),
        ("depth_sampling_stride", _i32),
        ("max_blocks", _i64),
        ("max_points", _i64),
    ]


HV_TRACK_MAX_LEVELS = 8
HV_TRACK_TRACE_STRIDE = 56


class HvTrackParams(_c.Structure):
    _fields_ = [
        ("depth_scale", _f64),
        ("depth_min", _f64),
        ("depth_max", _f64),
        ("weight_threshold", _f64),
        ("depth_outlier_trunc", _f64),
        ("depth_huber_delta", _f64),
        ("n_levels", _i32),
        ("iterations", _i32 * HV_TRACK_MAX_LEVELS),
    ]


class HvTrackResult(_c.Structure):
    _fields_ = [
        ("T_cw", _f64 * 16),
        ("information", _f64 * 36),
        ("fitness", _f64),
        ("inlier_rmse", _f64),
        ("inliers", _i64),
        ("valid", _i64),
        ("iterations", _i32 * HV_TRACK_MAX_LEVELS),
        ("degenerate", _i32),
        ("success", _i32),
    ]


HV_TRACK_COLOR_TRACE_STRIDE = 58


class HvTrackColorParams(_c.Structure):
    _fields_ = [("base", HvTrackParams), ("intensity_weight", _f64), ("intensity_huber_delta", _f64)]


class HvTrackColorResult(_c.Structure):
    _fields_ = [("base", HvTrackResult), ("photometric_inliers", _i64), ("intensity_rmse", _f64)]


HV_POSE_GRAPH_TRACE_STRIDE = 12
HV_POSE_GRAPH_RULES = {0: "max_iterations", 1: "gradient", 2: "step", 3: "decrease", 4: "residual"}


class HvPoseGraphParams(_c.Structure):
    _fields_ = [
        ("line_process_weight", _f64),
        ("edge_prune_threshold", _f64),
        ("lambda_scale", _f64),
        ("gradient_tolerance", _f64),
        ("step_tolerance", _f64),
        ("decrease_tolerance", _f64),
        ("residual_tolerance", _f64),
        ("cg_tolerance", _f64),
        ("max_iterations", _i32),
        ("cg_max_iterations", _i32),
        ("fixed", _i32),
        ("trace_state", _i32),
    ]


class HvPoseGraphResult(_c.Structure):
    _fields_ = [
        ("chi2_initial", _f64),
        ("chi2_final", _f64),
        ("lambda_", _f64),
        ("iterations", _i32),
        ("cg_iterations_total", _i32),
        ("edges_kept", _i32),
        ("converged", _i32),
        ("success", _i32),
    ]


class HvBundleParams(_c.Structure):
    _fields_ = [
        ("fx", _f64),
        ("fy", _f64),
        ("cx", _f64),
        ("cy", _f64),
        ("bf", _f64),
        ("huber_delta2_mono", _f64),
        ("huber_delta2_stereo", _f64),
        ("min_depth", _f64),
        ("lambda_scale", _f64),
        ("gradient_tolerance", _f64),
        ("step_tolerance", _f64),
        ("decrease_tolerance", _f64),
        ("residual_tolerance", _f64),
        ("cg_tolerance", _f64),
        ("max_iterations", _i32),
        ("cg_max_iterations", _i32),
        ("huber", _i32),
        ("fixed_points", _i32),
        ("trace_state", _i32),
        ("reserved", _i32),
    ]


class HvBundleResult(_c.Structure):
    _fields_ = [
        ("chi2_initial", _f64),
        ("chi2_final", _f64),
        ("lambda_", _f64),
        ("iterations", _i32),
        ("cg_iterations_total", _i32),
        ("converged", _i32),
        ("success", _i32),
    ]


class HvOdometryParams(_c.Structure):
    _fields_ = [
        ("depth_scale", _f64),
        ("depth_min", _f64),
        ("depth_max", _f64),
        ("depth_outlier_trunc", _f64),
        ("depth_huber_delta", _f64),
        ("intensity_weight", _f64),
        ("intensity_huber_delta", _f64),
        ("n_levels", _i32),
        ("iterations", _i32 * HV_TRACK_MAX_LEVELS),
    ]


class HvOdometryResult(_c.Structure):
    _fields_ = [
        ("transformation", _f64 * 16),
        ("information", _f64 * 36),
        ("fitness", _f64),
        ("inlier_rmse", _f64),
        ("inliers", _i64),
        ("valid", _i64),
        ("iterations", _i32 * HV_TRACK_MAX_LEVELS),
        ("degenerate", _i32),
        ("success", _i32),
        ("photometric_inliers", _i64),
        ("intensity_rmse", _f64),
    ]


HV_TSDF_DEINTEGRATE_MAX_FRAMES = 64


class HvDeintegrateStats(_c.Structure):
    _fields_ = [
        ("units_listed", _i64),
        ("units_missing", _i64),
        ("voxels_removed", _i64),
        ("voxels_underflow", _i64),
    ]


class HvPruneStats(_c.Structure):
    _fields_ = [
        ("units_before", _i64),
        ("units_outside", _i64),
        ("units_empty", _i64),
        ("units_after", _i64),
    ]


class HvMergeStats(_c.Structure):
    _fields_ = [
        ("units_source", _i64),
        ("units_claimed", _i64),
        ("voxels_updated", _i64),
        ("voxels_trilinear", _i64),
        ("voxels_nearest", _i64),
    ]


HV_REGISTER_TRACE_STRIDE = 54


class HvRegisterParams(_c.Structure):
    _fields_ = [
        ("weight_threshold", _f64),
        ("tsdf_band", _f64),
        ("residual_trunc", _f64),
        ("huber_delta", _f64),
        ("max_iterations", _i32),
        ("reserved", _i32),
    ]


class HvRegisterResult(_c.Structure):
    _fields_ = [
        ("T_dst_src", _f64 * 16),
        ("information", _f64 * 36),
        ("anchor", _f64 * 3),
        ("fitness", _f64),
        ("inlier_rmse", _f64),
        ("inliers", _i64),
        ("candidates", _i64),
        ("iterations", _i32),
        ("success", _i32),
    ]


HV_PACK_VERSION = 1
HV_PACK_HEADER_BYTES = 128


class HvPackInfo(_c.Structure):
    _fields_ = [("units", _i64), ("voxels", _i64), ("bytes", _i64)]


class HvPackedHeader(_c.Structure):
    _fields_ = [
        ("voxel_length", _f64),
        ("sdf_trunc", _f64),
        ("resolution", _i32),
        ("version", _i32),
        ("units", _i64),
        ("voxels", _i64),
        ("bytes", _i64),
    ]


HV_GRID_PACK_VERSION = 1
HV_GRID_PACK_HEADER_BYTES = 192


class HvGridPackInfo(_c.Structure):
    _fields_ = [("blocks", _i64), ("voxels", _i64), ("extra_pairs", _i64), ("bytes", _i64)]


class HvGridPackedHeader(_c.Structure):
    _fields_ = [
        ("voxel_size", _f64),
        ("mode", _i32),
        ("block_size", _i32),
        ("record_bytes", _i32),
        ("version", _i32),
        ("next_object_id", _i32),
        ("depth_threshold", _f32),
        ("depth_decay_rate", _f32),
        ("reserved", _i32),
        ("blocks", _i64),
        ("voxels", _i64),
        ("extra_pairs", _i64),
        ("bytes", _i64),
        ("chain_nodes", _i64),
    ]


HV_F32, HV_F64 = 0, 1
HV_SAMPLE_OUTSIDE, HV_SAMPLE_UNOBSERVED, HV_SAMPLE_NEAREST, HV_SAMPLE_TRILINEAR = 0, 1, 2, 3
HV_CHECK_INVALID, HV_CHECK_UNKNOWN, HV_CHECK_CONSISTENT, HV_CHECK_IN_FRONT, HV_CHECK_BEHIND = 0, 1, 2, 3, 4


class HvCheckParams(_c.Structure):
    _fields_ = [
        ("depth_scale", _f64),
        ("depth_min", _f64),
        ("depth_max", _f64),
        ("weight_threshold", _f64),
        ("tolerance", _f64),
    ]


class HvCheckStats(_c.Structure):
    _fields_ = [("count", _i64 * 5)]


HV_LOOKUP_MISSING, HV_LOOKUP_OWN, HV_LOOKUP_NEAR, HV_LOOKUP_INVALID = 0, 1, 2, 3


class HvLookupParams(_c.Structure):
    _fields_ = [("min_count", _i32), ("min_confidence", _f32), ("radius", _i32)]


class HvLookupStats(_c.Structure):
    _fields_ = [("points", _i64), ("own", _i64), ("near", _i64), ("missing", _i64), ("invalid", _i64)]


HV_DIST_UNKNOWN, HV_DIST_FREE, HV_DIST_INSIDE, HV_DIST_SITE = 0, 1, 2, 4
HV_DIST_MAX_SHAPE, HV_DIST_MAX_RADIUS = 4096, 1024


class HvDistanceParams(_c.Structure):
    _fields_ = [("origin", _i32 * 3), ("shape", _i32 * 3), ("radius", _i32), ("weight_threshold", _f64)]


class HvDistanceStats(_c.Structure):
    _fields_ = [("unknown", _i64), ("free", _i64), ("inside", _i64), ("sites", _i64), ("far", _i64)]


HV_COMPONENTS_MAX_MARGIN = 16


class HvComponentsStats(_c.Structure):
    _fields_ = [("units", _i64), ("sites", _i64), ("components", _i64), ("largest", _i64)]


class HvRemoveComponentsStats(_c.Structure):
    _fields_ = [("components", _i64), ("components_removed", _i64), ("sites", _i64), ("sites_removed", _i64), ("voxels_reset", _i64),
                ("units_changed", _i64), ("units_emptied", _i64)]


class HvStereoParams(_c.Structure):
    _fields_ = [("num_disparities", _i32), ("p1", _i32), ("p2", _i32), ("uniqueness_ratio", _i32), ("max_diff", _i32), ("paths", _i32),
                ("bf", _f32), ("min_depth", _f32), ("max_depth", _f32)]


class HvMvsParams(_c.Structure):
    _fields_ = [("num_planes", _i32), ("p1", _i32), ("p2", _i32), ("uniqueness_ratio", _i32), ("min_views", _i32), ("paths", _i32),
                ("min_depth", _f64), ("max_depth", _f64), ("speckle_window_size", _i32), ("speckle_range", _i32)]


class HvConsistencyParams(_c.Structure):
    _fields_ = [("max_reproj_error", _f32), ("inv_depth_tol", _f32), ("rel_depth_tol", _f32), ("min_consistent", _i32), ("max_violations", _i32),
                ("fuse", _i32)]


class HvConsistencyStats(_c.Structure):
    _fields_ = [("valid_pixels", _i64), ("kept_pixels", _i64), ("agree_sum", _i64)]


class HvFeatureParams(_c.Structure):
    _fields_ = [("levels", _i32), ("threshold", _i32), ("per_cell", _i32)]


class HvMatchParams(_c.Structure):
    _fields_ = [("max_distance", _i32), ("ratio_percent", _i32), ("cross_check", _i32)]


HV_SPECKLE_I16, HV_SPECKLE_F32 = 0, 1


class HvSpeckleStats(_c.Structure):
    _fields_ = [("valid_pixels", _i64), ("components", _i64), ("largest", _i64), ("removed_components", _i64), ("removed_pixels", _i64)]


# name -> (restype, argtypes); mirrors include/hipvol.h one to one
SIGNATURES = {
    "hv_last_error": (_c.c_char_p, []),
    "hv_device_count": (_i32, []),
    "hv_default_config": (None, [_i32, _c.POINTER(HvConfig)]),
    "hv_create": (_i32, [_c.POINTER(HvConfig), _c.POINTER(_vp)]),
    "hv_destroy": (None, [_vp]),
    "hv_reset": (_i32, [_vp]),
    "hv_synchronize": (_i32, [_vp]),
    "hv_set_stream": (_i32, [_vp, _vp]),
    "hv_get_stream": (_vp, [_vp]),
    "hv_num_blocks": (_i32, [_vp, _pi64]),
    "hv_block_size": (_i32, [_vp, _pi32]),
    "hv_reserve_blocks": (_i32, [_vp, _i64]),
    "hv_max_blocks": (_i32, [_vp, _pi64]),
    "hv_bytes_per_block": (_i32, [_vp, _pi64]),
    "hv_dropped_points": (_i32, [_vp, _pi64]),
    "hv_integrate_points": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32]),
    "hv_integrate_points_f64": (_i32, [_vp, _vp, _i64, _vp, _i32, _i32]),
    "hv_integrate_rgbd_points": (_i32, [_vp, _vp, _i32, _f64, _vp, _i32, _i32, _vp, _vp, _f64, _f64, _i32]),
    "hv_integrate_rgbd_points_batch": (_i32, [_vp, _vp, _i32, _f64, _vp, _i32, _i32, _i32, _vp, _vp, _f64, _f64, _i32]),
    "hv_remap": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _i32]),
    "hv_filter_shadow_points": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _i32]),
    "hv_filter_shadow_points_on_stream": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "hv_stereo_sgm": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _c.POINTER(HvStereoParams), _vp, _vp, _i32]),
    "hv_filter_speckles": (_i32, [_vp, _vp, _i32, _i32, _i32, _f64, _i64, _f64, _vp, _vp, _vp, _c.POINTER(HvSpeckleStats), _i32]),
    "hv_stereo_sgm_speckle": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _c.POINTER(HvStereoParams), _i32, _i32, _vp, _vp,
                                     _c.POINTER(HvSpeckleStats), _i32]),
    "hv_mvs_sgm": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _c.POINTER(HvMvsParams), _vp, _vp, _c.POINTER(HvSpeckleStats), _i32]),
    "hv_depth_consistency": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _c.POINTER(HvConsistencyParams), _vp, _vp,
                                    _c.POINTER(HvConsistencyStats), _i32]),
    "hv_get_voxels": (_i32, [_vp, _i32, _f32, _vp, _vp, _i64, _pi64, _i32]),
    "hv_get_voxels_in_bb": (_i32, [_vp, _vp, _i32, _f32, _vp, _vp, _i64, _pi64, _i32]),
    "hv_get_voxels_in_frustum": (_i32, [_vp, _vp, _i32, _i32, _vp, _f32, _f32, _i32, _f32, _vp, _vp, _i64, _pi64, _i32]),
    "hv_carve": (_i32, [_vp, _vp, _i32, _i32, _vp, _f32, _f32, _vp, _f32, _i32]),
    "hv_remove_low_count_voxels": (_i32, [_vp, _i32]),
    "hv_size": (_i32, [_vp, _pi64]),
    "hv_dump_blocks": (_i32, [_vp, _vp, _vp, _vp, _vp, _pi64]),
    "hv_keys_from_points": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "hv_integrate_points_semantic": (_i32, [_vp, _vp, _i32, _i64, _vp, _i32, _vp, _vp, _vp, _i32]),
    "hv_get_voxels_semantic": (_i32, [_vp, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _pi64]),
    "hv_get_voxels_semantic_in_bb": (_i32, [_vp, _vp, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _pi64]),
    "hv_get_voxels_semantic_in_frustum": (_i32, [_vp, _vp, _i32, _i32, _vp, _f32, _f32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i64, _pi64]),
    "hv_set_depth_threshold": (_i32, [_vp, _f32]),
    "hv_dump_blocks_semantic": (_i32, [_vp, _vp, _vp, _vp, _vp, _pi64]),
    "hv_dump_blocks_semantic2": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _pi64]),
    "hv_dump_marginals_semantic": (_i32, [_vp, _vp, _vp, _pi64]),
    "hv_set_depth_decay_rate": (_i32, [_vp, _f32]),
    "hv_integrate_rgbd_semantic": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _f64, _f64, _i32, _i32]),
    "hv_label_overflows": (_i32, [_vp, _pi64]),
    "hv_prob_nodes_used": (_i32, [_vp, _pi64]),
    "hv_assign_object_ids_to_instance_ids": (_i32, [_vp, _vp, _i32, _i32, _vp, _f32, _f32, _vp, _vp, _vp, _f32, _i32, _f32, _i32,
                                                    _vp, _vp, _i64, _pi64, _i32]),
    "hv_assoc_vote": (_i32, [_vp, _vp, _i32, _i32, _vp, _f32, _f32, _vp, _vp, _vp, _f32, _i32, _i32]),
    "hv_assoc_pairs_fetch": (_i32, [_vp, _vp, _vp, _i64, _pi64]),
    "hv_assoc_pairs_set": (_i32, [_vp, _vp, _vp, _i64]),
    "hv_assoc_pairs_export": (_i32, [_vp, _vp, _i64]),
    "hv_assoc_pairs_import": (_i32, [_vp, _vp, _i32, _i64]),
    "hv_assoc_decide": (_i32, [_vp, _f32, _i32]),
    "hv_assoc_map_fetch": (_i32, [_vp, _vp, _vp, _i64, _pi64]),
    "hv_remap_instance_ids_last": (_i32, [_vp, _vp, _i32, _i32, _vp, _i32]),
    "hv_semantic_fuse_keyframe": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _f32, _f32, _vp, _vp, _i32, _i32, _f32, _i32, _f32, _i32,
                                         _f64, _f64, _i32]),
    "hv_peek_next_object_id": (_i32, []),
    "hv_set_next_object_id": (None, [_i32]),
    "hv_remap_instance_ids": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _vp, _i32]),
    "hv_object_segments_compute": (_i32, [_vp, _i32, _f32, _pi64, _pi64]),
    "hv_object_segments_fetch": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "hv_compute_obb_pca": (_i32, [_vp, _i64, _vp]),
    "hv_merge_segments": (_i32, [_vp, _i32, _i32]),
    "hv_remove_segment": (_i32, [_vp, _i32]),
    "hv_remove_low_confidence_segments": (_i32, [_vp, _i32]),
    "hv_remove_low_confidence_voxels": (_i32, [_vp, _f32]),
    "hv_tsdf_integrate": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _f64, _f64, _i32]),
    "hv_tsdf_integrate_batch": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _f64, _f64, _i32]),
    "hv_tsdf_integrate_frames": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _f64, _f64]),
    "hv_tsdf_set_color_order": (_i32, [_vp, _i32]),
    "hv_host_register": (_i32, [_vp, _i64]),
    "hv_host_unregister": (_i32, [_vp]),
    "hv_tsdf_set_tile": (_i32, [_vp, _i32, _i32, _i32, _i32]),
    "hv_tsdf_set_rectify_maps": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32]),
    "hv_tsdf_set_owner": (_i32, [_vp, _i32, _i32]),
    "hv_tsdf_extract_mesh": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _pi64, _pi64]),
    "hv_tsdf_extract_mesh_f32": (_i32, [_vp, _vp, _vp, _i64, _vp, _i64, _pi64, _pi64]),
    "hv_tsdf_extract_mesh_clustered": (_i32, [_vp, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _pi64, _pi64, _pi64]),
    "hv_tsdf_extract_mesh_clustered_f32": (_i32, [_vp, _i32, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _pi64, _pi64, _pi64]),
    "hv_tsdf_extract_points": (_i32, [_vp, _vp, _vp, _i64, _pi64]),
    "hv_tsdf_extract_points_f32": (_i32, [_vp, _vp, _vp, _i64, _pi64]),
    "hv_tsdf_extract_point_normals": (_i32, [_vp, _vp, _i64, _pi64]),
    "hv_tsdf_ray_cast": (_i32, [_vp, _i32, _i32, _vp, _vp, _f64, _f64, _f64, _f64, _vp, _vp, _vp, _vp, _vp, _i32]),
    "hv_tsdf_deintegrate": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _f64, _f64, _i32, _c.POINTER(HvDeintegrateStats)]),
    "hv_tsdf_deintegrate_batch": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _f64, _f64, _i32, _c.POINTER(HvDeintegrateStats)]),
    "hv_tsdf_reintegrate_batch": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _f64, _f64, _i32,
                                         _c.POINTER(HvDeintegrateStats)]),
    "hv_tsdf_prune": (_i32, [_vp, _i32, _pi32, _pi32, _c.POINTER(HvPruneStats)]),
    "hv_tsdf_integrate_volume": (_i32, [_vp, _vp, _vp, _c.POINTER(HvMergeStats)]),
    "hv_tsdf_register_volume": (_i32, [_vp, _vp, _vp, _c.POINTER(HvRegisterParams), _c.POINTER(HvRegisterResult), _vp, _i64, _pi64]),
    "hv_tsdf_track": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _pi64, _i32]),
    "hv_tsdf_track_color": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _pi64, _i32]),
    "hv_rgbd_odometry": (_i32, [_vp, _vp, _vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _pi64, _i32]),
    "hv_rgbd_odometry_model": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _i32]),
    "hv_pose_graph_default_params": (None, [_c.POINTER(HvPoseGraphParams)]),
    "hv_pose_graph_optimize": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _c.POINTER(HvPoseGraphParams), _vp, _c.POINTER(HvPoseGraphResult),
                                      _vp, _vp, _i64, _pi64, _i32]),
    "hv_pose_graph_linearise": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _f64, _vp, _vp, _vp, _vp, _vp, _vp, _i32]),
    "hv_bundle_default_params": (None, [_c.POINTER(HvBundleParams)]),
    "hv_bundle_adjust": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _c.POINTER(HvBundleParams), _vp, _vp, _c.POINTER(HvBundleResult),
                                _vp, _vp, _vp, _i64, _pi64, _i32]),
    "hv_bundle_linearise": (_i32, [_vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _c.POINTER(HvBundleParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _i32]),
    "hv_orb_detect": (_i32, [_vp, _vp, _i32, _i32, _i32, _c.POINTER(HvFeatureParams), _vp, _vp, _i64, _pi32, _i32]),
    "hv_match_descriptors": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _c.POINTER(HvMatchParams), _vp, _vp, _vp, _vp, _i32]),
    "hv_tsdf_sample_points": (_i32, [_vp, _vp, _i32, _i64, _f64, _vp, _vp, _vp, _vp, _vp, _i32]),
    "hv_tsdf_check_frame": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _c.POINTER(HvCheckParams), _vp, _vp, _c.POINTER(HvCheckStats), _i32]),
    "hv_lookup_points": (_i32, [_vp, _vp, _i32, _i64, _c.POINTER(HvLookupParams), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _c.POINTER(HvLookupStats), _i32]),
    "hv_tsdf_distance_field": (_i32, [_vp, _c.POINTER(HvDistanceParams), _vp, _vp, _vp, _c.POINTER(HvDistanceStats), _i32]),
    "hv_tsdf_surface_components": (_i32, [_vp, _f64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _pi64, _pi64, _c.POINTER(HvComponentsStats), _i32]),
    "hv_tsdf_remove_components": (_i32, [_vp, _f64, _i64, _i32, _c.POINTER(HvRemoveComponentsStats)]),
    "hv_tsdf_dump": (_i32, [_vp, _vp, _vp, _vp, _vp, _pi64]),
    "hv_tsdf_touched": (_i32, [_vp, _vp, _i64, _pi64]),
    "hv_tsdf_export_numerators": (_i32, [_vp, _vp, _i64, _vp, _i32]),
    "hv_tsdf_import_numerators": (_i32, [_vp, _vp, _i64, _vp, _i32]),
    "hv_tsdf_unit_keys": (_i32, [_vp, _vp, _i64, _pi64]),
    "hv_tsdf_pack_size": (_i32, [_vp, _c.POINTER(HvPackInfo)]),
    "hv_tsdf_pack": (_i32, [_vp, _vp, _i64, _i32, _c.POINTER(HvPackInfo)]),
    "hv_tsdf_unpack": (_i32, [_vp, _vp, _i64, _i32, _c.POINTER(HvPackInfo)]),
    "hv_tsdf_packed_check": (_i32, [_vp, _i64, _c.POINTER(HvPackedHeader)]),
    "hv_grid_pack_size": (_i32, [_vp, _c.POINTER(HvGridPackInfo)]),
    "hv_grid_pack": (_i32, [_vp, _vp, _i64, _i32, _c.POINTER(HvGridPackInfo)]),
    "hv_grid_unpack": (_i32, [_vp, _vp, _i64, _i32, _c.POINTER(HvGridPackInfo)]),
    "hv_grid_packed_check": (_i32, [_vp, _i64, _c.POINTER(HvGridPackedHeader)]),
    "hv_tsdf_dirty_keys": (_i32, [_vp, _vp, _i64, _pi64]),
    "hv_tsdf_mark_merged": (_i32, [_vp]),
    "hv_set_owner": (_i32, [_vp, _i32, _i32]),
    "hv_block_owner": (_i32, [_vp, _i64, _i32, _vp]),
    "hv_merge_halo_plan": (_i32, [_vp, _vp, _i32, _i32, _vp, _vp, _i64, _pi64]),
    "hv_merge_halo_plan_held": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _pi64]),
    "hv_merge_halo_pack": (_i32, [_vp, _vp, _i64, _vp, _i32]),
    "hv_merge_halo_unpack": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32]),
    "hv_merge_halo_lists_device": (_i32, [_vp, _vp, _i64, _vp, _i64, _pi64, _pi64]),
    "hv_merge_halo_plan_device": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _pi64]),
    "hv_merge_halo_plan_fetch": (_i32, [_vp, _vp, _vp, _i64, _pi64]),
    "hv_merge_halo_pack_planned": (_i32, [_vp, _i64, _i64, _vp]),
    "hv_merge_halo_unpack_planned": (_i32, [_vp, _i64, _i64, _vp]),
    "hv_profile_enable": (_i32, [_vp, _i32]),
    "hv_profile_read": (_i32, [_vp, _c.POINTER(_f64), _pi64, _pi64]),
    "hv_profile_read_launches": (_i32, [_vp, _vp, _i64, _pi64]),
}

_lib = None


class HipVolError(RuntimeError):
    """Raised for every non-zero hv_status; message = hv_last_error()."""


def library_path():
    return _build.LIB_PATH


def load():
    """Load (building if needed) libpyslam_hipvol.so and bind every symbol of include/hipvol.h."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if not os.path.exists(path):
        _build.build(verbose=False)
    # One HIP runtime per process: PyTorch-ROCm dlopens its bundled libamdhip64/libhsa-runtime64 by
    # absolute path, so if this library pulled in /opt/rocm's copies first the process would hold
    # two HSA runtimes and whichever initialises second sees no devices.  Importing torch first
    # makes our DT_NEEDED libamdhip64.so.7 resolve to the already-loaded runtime, which is also
    # what lets torch CUDA tensors and torch streams be passed straight into the C ABI.
    import torch  # noqa: F401

    lib = _c.CDLL(path)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(rc):
    if rc != HV_OK:
        msg = load().hv_last_error()
        raise HipVolError(msg.decode() if msg else f"hipvol error {rc}")


def ptr(a):
    """Device or host address of a numpy array / torch tensor / None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(_vp)
    if hasattr(a, "data_ptr"):
        return _vp(a.data_ptr())
    raise TypeError(f"unsupported buffer type {type(a)}")


def location(a):
    """HV_DEVICE for torch tensors living on a GPU, HV_HOST otherwise."""
    if a is not None and hasattr(a, "is_cuda") and a.is_cuda:
        return HV_DEVICE
    return HV_HOST
