"""ctypes binding of liborbx.so (include/orbx.h).

The HIP library is the product: if it is missing this module raises instead of
falling back to any CPU path.
"""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import numpy as np

import os

# ORBX_LIB: alternative build of the library (A/B measurements of kernel variants)
LIB_PATH = Path(os.environ.get("ORBX_LIB", str(Path(__file__).resolve().parent / "liborbx.so")))

ORBX_OK = 0
ORBX_EMPTY = 1
ORBX_ERR_ARG = -1
ORBX_ERR_HIP = -2
ORBX_ERR_CAPACITY = -3
ORBX_ERR_UNSUPPORTED = -4
ORBX_ERR_STATE = -5

# == cv::KeyPoint / orbx_keypoint (28 bytes)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])

EXPORTED = [
    "orbx_extractor_create", "orbx_extractor_destroy", "orbx_extractor_levels",
    "orbx_extractor_features_per_level", "orbx_extractor_max_keypoints", "orbx_extract",
    "orbx_extract_batch", "orbx_extract_batch_device", "orbx_extractor_stream", "orbx_extractor_set_stage_event",
    "orbx_stream_wait_event", "orbx_stream_create", "orbx_stream_destroy",
    "orbx_extractor_set_timing", "orbx_extractor_stage_times", "orbx_pyramid_level",
    "orbx_pyramid_level_device", "orbx_hamming", "orbx_hamming_matrix_device",
    "orbx_window_match_device", "orbx_window_match", "orbx_version", "orbx_device_count",
    "orbx_last_error", "orbx_matcher_create", "orbx_matcher_destroy", "orbx_search_by_projection_local",
    "orbx_search_by_projection_frame", "orbx_search_for_triangulation", "orbx_compute_stereo_matches",
    "orbx_match_sequence_device", "orbx_matcher_set_timing", "orbx_matcher_last_ms", "orbx_matcher_last_call_us",
    "orbx_search_by_projection_keyframe", "orbx_search_by_projection_sim3", "orbx_matcher_set_footprint",
    "orbx_vocabulary_load_text_file", "orbx_vocabulary_load_text", "orbx_vocabulary_destroy",
    "orbx_vocabulary_info", "orbx_vocabulary_stream", "orbx_vocabulary_transform_features",
    "orbx_vocabulary_transform", "orbx_vocabulary_transform_batch_device", "orbx_vocabulary_set_timing",
    "orbx_vocabulary_stage_times", "orbx_search_by_bow_frame", "orbx_search_by_bow_keyframes",
    "orbx_search_for_initialization", "orbx_undistort_keypoints", "orbx_undistort_keypoints_device",
    "orbx_compute_image_bounds", "orbx_assign_features_to_grid", "orbx_assign_features_to_grid_device",
    "orbx_fuse", "orbx_fuse_sim3", "orbx_search_by_sim3", "orbx_compute_distinctive_descriptors",
    "orbx_compute_distinctive_descriptors_device", "orbx_extractor_status", "orbx_extractor_status_device",
    "orbx_extractor_set_node_capacity", "orbx_extractor_set_level0_in_place", "orbx_compute_stereo_matches_batch_device",
    "orbx_search_for_triangulation_batch_device", "orbx_match_sequence_device_ex",
    "orbx_search_local_points_device", "orbx_create_mappoints_device", "orbx_update_last_frame_device",
    "orbx_extractor_last_call_us", "orbx_compute_stereo_from_rgbd", "orbx_compute_stereo_from_rgbd_device",
    "orbx_debug_set", "orbx_bow_score", "orbx_kfdb_create", "orbx_kfdb_destroy", "orbx_kfdb_info", "orbx_kfdb_stream",
    "orbx_kfdb_add_batch_device", "orbx_kfdb_add", "orbx_kfdb_erase", "orbx_kfdb_clear", "orbx_kfdb_set_covisibility",
    "orbx_kfdb_reloc_scores", "orbx_kfdb_score_device", "orbx_kfdb_detect_relocalization_candidates_device",
    "orbx_kfdb_detect_loop_candidates_device", "orbx_kfdb_detect_relocalization_candidates",
    "orbx_kfdb_detect_loop_candidates", "orbx_pose_optimization_batch_device", "orbx_pose_optimization",
    "orbx_sim3_create", "orbx_sim3_destroy", "orbx_sim3_set_batch_device", "orbx_sim3_iterate_device", "orbx_sim3_set",
    "orbx_sim3_iterate", "orbx_sim3_draws", "orbx_pnp_create", "orbx_pnp_destroy", "orbx_pnp_set_batch_device",
    "orbx_pnp_iterate_device", "orbx_pnp_set", "orbx_pnp_iterate", "orbx_pnp_draws", "orbx_optimize_sim3_batch_device", "orbx_optimize_sim3",
    "orbx_triangulate_pairs_batch_device", "orbx_triangulate_pairs",
    "orbx_local_bundle_adjustment_batch_device", "orbx_local_bundle_adjustment",
    "orbx_global_bundle_adjustment_batch_device", "orbx_global_bundle_adjustment", "orbx_global_ba_envelope",
    "orbx_optimize_essential_graph_batch_device", "orbx_optimize_essential_graph", "orbx_essential_graph_envelope",
    "orbx_initializer_create", "orbx_initializer_destroy", "orbx_initializer_initialize_device",
    "orbx_initializer_initialize", "orbx_initializer_sets",
    "orbx_covis_create", "orbx_covis_destroy", "orbx_covis_stream", "orbx_covis_refresh_observations_device",
    "orbx_covis_update_connections_device", "orbx_covis_erase_keyframe_device", "orbx_covis_view_device",
    "orbx_covis_best_covisibles_device", "orbx_covis_covisibles_by_weight_device", "orbx_covis_ordered",
    "orbx_covis_read", "orbx_covis_refresh_observations", "orbx_local_ba_assemble_device", "orbx_local_ba_apply_device",
    "orbx_update_local_map_device", "orbx_update_local_map", "orbx_search_local_points_offsets_device",
    "orbx_track_local_map_tally_device",
    "orbx_keyframe_culling_device", "orbx_covis_set_bad_flag_device", "orbx_map_point_culling_device",
    "orbx_covis_observation_counts_device", "orbx_update_normal_and_depth_device",
    "orbx_correct_loop_propagate_device", "orbx_essential_graph_assemble_device",
]

ORBX_DEPTH_U16 = 0
ORBX_DEPTH_F32 = 1


class Camera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k1", C.c_float),
                ("k2", C.c_float), ("p1", C.c_float), ("p2", C.c_float), ("k3", C.c_float)]


class ExtractorParams(C.Structure):
    _fields_ = [("nfeatures", C.c_int), ("scale_factor", C.c_float), ("nlevels", C.c_int),
                ("ini_th_fast", C.c_int), ("min_th_fast", C.c_int)]


class Sequence(C.Structure):
    """orbx_sequence (include/orbx.h)."""
    _fields_ = [("batch", C.c_int), ("kps", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_void_p), ("cap", C.c_int),
                ("Tcw", C.c_void_p), ("u_right", C.c_void_p), ("mp_pos", C.c_void_p), ("has_mp", C.c_void_p),
                ("depth", C.c_float), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("bf", C.c_float), ("b", C.c_float), ("min_x", C.c_float), ("max_x", C.c_float),
                ("min_y", C.c_float), ("max_y", C.c_float), ("nlevels", C.c_int),
                ("scale_factors", C.POINTER(C.c_float)), ("th", C.c_float), ("mono", C.c_int),
                ("global_ids", C.c_int), ("cur_mp", C.c_void_p), ("nmatches", C.c_void_p), ("mp_obs", C.c_void_p),
                ("retry_below", C.c_int)]


class RgbdBatch(C.Structure):
    """orbx_rgbd_batch (include/orbx.h)."""
    _fields_ = [("batch", C.c_int), ("kps", C.c_void_p), ("kps_un", C.c_void_p), ("n", C.c_void_p), ("cap", C.c_int),
                ("depth", C.c_void_p), ("depth_type", C.c_int), ("width", C.c_int), ("height", C.c_int),
                ("row_bytes", C.c_longlong), ("frame_bytes", C.c_longlong), ("depth_map_factor", C.c_float),
                ("bf", C.c_float), ("u_right", C.c_void_p), ("depth_out", C.c_void_p)]


class MapPointsDevice(C.Structure):
    """orbx_mappoints_device."""
    _fields_ = [("n", C.c_int), ("pos", C.c_void_p), ("desc", C.c_void_p), ("normal", C.c_void_p),
                ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("observations", C.c_void_p),
                ("bad", C.c_void_p)]


class LocalMapBatch(C.Structure):
    """orbx_local_map_batch."""
    _fields_ = [("batch", C.c_int), ("kps", C.c_void_p), ("desc", C.c_void_p), ("n", C.c_void_p), ("cap", C.c_int),
                ("u_right", C.c_void_p), ("Tcw", C.c_void_p), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("min_x", C.c_float),
                ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float), ("nlevels", C.c_int),
                ("scale_factors", C.POINTER(C.c_float)), ("local_off", C.POINTER(C.c_int32)),
                ("local_ids", C.c_void_p), ("th", C.c_float), ("viewing_cos_limit", C.c_float),
                ("frame_mp", C.c_void_p), ("nmatches", C.c_void_p)]


class PoseOptimizationBatch(C.Structure):
    """orbx_pose_optimization_batch."""
    _fields_ = [("batch", C.c_int), ("kps", C.c_void_p), ("n", C.c_void_p), ("cap", C.c_int),
                ("u_right", C.c_void_p), ("frame_mp", C.c_void_p), ("n_mp", C.c_int), ("mp_pos", C.c_void_p),
                ("inv_level_sigma2", C.POINTER(C.c_float)), ("nlevels", C.c_int), ("fx", C.c_float),
                ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float), ("Tcw", C.c_void_p),
                ("Tcw_opt", C.c_void_p), ("outlier", C.c_void_p), ("ninliers", C.c_void_p), ("ninit", C.c_void_p),
                ("trace", C.c_void_p), ("discard_outliers", C.c_int), ("mp_obs", C.c_void_p),
                ("nmatches_map", C.c_void_p)]


ORBX_POSE_OPT_LDS_EDGES = 1984


class Sim3Batch(C.Structure):
    """orbx_sim3_batch."""
    _fields_ = [("batch", C.c_int), ("cap", C.c_int), ("n1", C.c_void_p), ("mp1", C.c_void_p), ("mp2", C.c_void_p),
                ("oct1", C.c_void_p), ("oct2", C.c_void_p), ("n_mp", C.c_int), ("mp_pos", C.c_void_p),
                ("Tcw1", C.c_void_p), ("Tcw2", C.c_void_p), ("level_sigma2", C.POINTER(C.c_float)),
                ("nlevels", C.c_int), ("K1", C.POINTER(C.c_float)), ("K2", C.POINTER(C.c_float)),
                ("fix_scale", C.c_int), ("probability", C.c_double), ("min_inliers", C.c_int),
                ("max_iterations", C.c_int), ("draws", C.c_void_p)]


class Sim3Result(C.Structure):
    """orbx_sim3_result."""
    _fields_ = [(k, C.c_void_p) for k in ("found", "no_more", "n_inliers", "inliers", "T12", "best_R", "best_t",
                                          "best_s", "best_inliers", "best_iteration", "iterations", "n_pairs",
                                          "status")]


ORBX_SIM3_MAX_ITERATIONS = 4096
ORBX_SIM3_STATUS_BAD_DRAW = 1


class PnpBatch(C.Structure):
    """orbx_pnp_batch."""
    _fields_ = [("batch", C.c_int), ("cap", C.c_int), ("kps", C.c_void_p), ("n", C.c_void_p), ("matches", C.c_void_p),
                ("n_mp", C.c_int), ("mp_pos", C.c_void_p), ("level_sigma2", C.POINTER(C.c_float)),
                ("nlevels", C.c_int), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("probability", C.c_double), ("min_inliers", C.c_int), ("max_iterations", C.c_int),
                ("min_set", C.c_int), ("epsilon", C.c_float), ("th2", C.c_float), ("draws", C.c_void_p),
                ("n_draws", C.c_int)]


PNP_RESULT_FIELDS = ("found", "no_more", "n_inliers", "inliers", "Tcw", "frame_mp", "best_Tcw", "best_inliers",
                     "best_iteration", "refined", "iterations", "n_corr", "min_inliers_used", "max_its_used",
                     "status")


class PnpResult(C.Structure):
    """orbx_pnp_result."""
    _fields_ = [(k, C.c_void_p) for k in PNP_RESULT_FIELDS]


ORBX_PNP_MAX_DRAWS = 4096
ORBX_PNP_STATUS_BAD_DRAW = 1
ORBX_PNP_STATUS_NO_DRAWS = 2


class OptimizeSim3Batch(C.Structure):
    """orbx_optimize_sim3_batch."""
    _fields_ = [("batch", C.c_int), ("cap1", C.c_int), ("n1", C.c_void_p), ("kps1", C.c_void_p), ("mp1", C.c_void_p),
                ("matches12", C.c_void_p), ("idx2", C.c_void_p), ("cap2", C.c_int), ("n2", C.c_void_p),
                ("kps2", C.c_void_p), ("n_mp", C.c_int), ("mp_pos", C.c_void_p), ("Tcw1", C.c_void_p),
                ("Tcw2", C.c_void_p), ("inv_level_sigma2_1", C.POINTER(C.c_float)),
                ("inv_level_sigma2_2", C.POINTER(C.c_float)), ("nlevels", C.c_int), ("K1", C.POINTER(C.c_float)),
                ("K2", C.POINTER(C.c_float)), ("R12", C.c_void_p), ("t12", C.c_void_p), ("s12", C.c_void_p),
                ("th2", C.c_float), ("fix_scale", C.c_int), ("R12_opt", C.c_void_p), ("t12_opt", C.c_void_p),
                ("s12_opt", C.c_void_p), ("ninliers", C.c_void_p), ("ncorr", C.c_void_p), ("nbad", C.c_void_p),
                ("trace", C.c_void_p)]


class LocalBaBatch(C.Structure):
    """orbx_local_ba_batch."""
    _fields_ = [("batch", C.c_int), ("kf_off", C.c_void_p), ("n_kf", C.c_int), ("kf_Tcw", C.c_void_p),
                ("kf_fixed", C.c_void_p), ("kf_slot", C.c_void_p), ("pt_off", C.c_void_p), ("n_pt", C.c_int),
                ("pt_pos", C.c_void_p), ("obs_off", C.c_void_p), ("n_obs", C.c_int), ("obs_kf", C.c_void_p),
                ("obs_kp", C.c_void_p), ("n_slots", C.c_int), ("cap", C.c_int), ("kps", C.c_void_p),
                ("u_right", C.c_void_p), ("inv_level_sigma2", C.POINTER(C.c_float)), ("nlevels", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("max_free_kf", C.c_int), ("kf_Tcw_opt", C.c_void_p), ("pt_pos_opt", C.c_void_p), ("erase", C.c_void_p),
                ("level1", C.c_void_p), ("n_erase", C.c_void_p), ("trace", C.c_void_p), ("status", C.c_void_p)]


ORBX_LOCAL_BA_MAX_FREE_KF = 64
ORBX_LOCAL_BA_STATUS_CAPACITY = 1
ORBX_LOCAL_BA_STATUS_NO_FREE_KF = 2
ORBX_LOCAL_BA_STATUS_BAD_INDEX = 4


class GlobalBaBatch(C.Structure):
    """orbx_global_ba_batch."""
    _fields_ = [("batch", C.c_int), ("kf_off", C.c_void_p), ("n_kf", C.c_int), ("kf_Tcw", C.c_void_p),
                ("kf_fixed", C.c_void_p), ("kf_slot", C.c_void_p), ("pt_off", C.c_void_p), ("n_pt", C.c_int),
                ("pt_pos", C.c_void_p), ("obs_off", C.c_void_p), ("n_obs", C.c_int), ("obs_kf", C.c_void_p),
                ("obs_kp", C.c_void_p), ("n_slots", C.c_int), ("cap", C.c_int), ("kps", C.c_void_p),
                ("u_right", C.c_void_p), ("inv_level_sigma2", C.POINTER(C.c_float)), ("nlevels", C.c_int),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("iterations", C.c_int), ("robust", C.c_int), ("max_env_blocks", C.c_int64), ("dense", C.c_int),
                ("kf_Tcw_opt", C.c_void_p), ("pt_pos_opt", C.c_void_p), ("pt_included", C.c_void_p),
                ("trace", C.c_void_p), ("chi2", C.c_void_p), ("status", C.c_void_p)]


ORBX_GLOBAL_BA_STATUS_CAPACITY = 1
ORBX_GLOBAL_BA_STATUS_NO_FREE_KF = 2
ORBX_GLOBAL_BA_STATUS_BAD_INDEX = 4


class EssentialGraphBatch(C.Structure):
    """orbx_essential_graph_batch."""
    _fields_ = [("batch", C.c_int), ("kf_off", C.c_void_p), ("n_kf", C.c_int), ("kf_Tcw", C.c_void_p),
                ("kf_corr", C.c_void_p), ("corr_S", C.c_void_p), ("n_corr", C.c_int), ("loop_kf", C.c_void_p),
                ("edge_off", C.c_void_p), ("n_edges", C.c_int), ("edge_v", C.c_void_p), ("edge_kind", C.c_void_p),
                ("pt_off", C.c_void_p), ("n_pt", C.c_int), ("pt_pos", C.c_void_p), ("pt_ref", C.c_void_p),
                ("fix_scale", C.c_int), ("iterations", C.c_int), ("max_env_blocks", C.c_int64), ("dense", C.c_int),
                ("kf_Tcw_opt", C.c_void_p), ("pt_pos_opt", C.c_void_p), ("Scw_opt", C.c_void_p), ("trace", C.c_void_p),
                ("chi2", C.c_void_p), ("status", C.c_void_p)]


ORBX_ESSENTIAL_GRAPH_STATUS_CAPACITY = 1
ORBX_ESSENTIAL_GRAPH_STATUS_NO_FIXED_KF = 2
ORBX_ESSENTIAL_GRAPH_STATUS_BAD_INDEX = 4


class KeyFrameGeomDevice(C.Structure):
    """orbx_keyframe_geom_device: device pointers (host ones in orbx_triangulate_pairs) + the host pose."""
    _fields_ = [("keys_un", C.c_void_p), ("keys", C.c_void_p), ("u_right", C.c_void_p), ("depth", C.c_void_p),
                ("n", C.c_void_p), ("Tcw", C.c_float * 12)]


class NewMapPoints(C.Structure):
    """orbx_new_mappoints: the outputs of the triangulation, every one nullable."""
    _fields_ = [(k, C.c_void_p) for k in ("reason", "method", "pos", "normal", "max_distance", "min_distance",
                                          "nnew", "new_idx")]


ORBX_TRIANGULATE_REASONS = ("accepted", "no branch", "w == 0", "z1 <= 0", "z2 <= 0", "reprojection KF1",
                            "reprojection KF2", "distance 0", "scale ratio", "bad index")


class InitializerBatch(C.Structure):
    """orbx_initializer_batch."""
    _fields_ = [("batch", C.c_int), ("kcap", C.c_int), ("n1", C.c_void_p), ("n2", C.c_void_p), ("keys1", C.c_void_p),
                ("keys2", C.c_void_p), ("matches12", C.c_void_p), ("K", C.POINTER(C.c_float)), ("sigma", C.c_float),
                ("max_iterations", C.c_int), ("sets", C.c_void_p)]


INITIALIZER_RESULT_FIELDS = ("ok", "model", "n_matches", "SH", "SF", "RH", "best_it_H", "best_it_F", "H21", "F21",
                             "inliers_H", "inliers_F", "n_inliers_H", "n_inliers_F", "R21", "t21", "p3d",
                             "triangulated", "best_good", "second_good", "n_similar", "parallax", "status")


class InitializerResult(C.Structure):
    """orbx_initializer_result: every output nullable."""
    _fields_ = [(k, C.c_void_p) for k in INITIALIZER_RESULT_FIELDS]


ORBX_INIT_MAX_ITERATIONS = 4096
ORBX_INIT_STATUS_BAD_SET = 1
ORBX_INIT_STATUS_TOO_FEW = 2


ORBX_COVIS_MAX_CONN = 8192
ORBX_COVIS_LDS_KEYFRAMES = 8192
ORBX_COVIS_STATUS_CAPACITY = 1
ORBX_COVIS_STATUS_BAD_KEYFRAME = 2
ORBX_COVIS_STATUS_DUPLICATE = 4


class CovisView(C.Structure):
    """orbx_covis_view."""
    _fields_ = [(k, C.c_int) for k in ("max_keyframes", "cap", "max_mappoints", "max_conn", "n_keyframes",
                                       "n_mappoints")] + \
               [(k, C.c_void_p) for k in ("obs_off", "obs_kf", "obs_idx", "mp", "row_kf", "row_w", "row_n",
                                          "ordered_kf", "ordered_w", "ordered_n", "parent", "first", "status")]


class LocalBaAssembly(C.Structure):
    """orbx_local_ba_assembly."""
    _fields_ = [("batch", C.c_int), ("cur_kf", C.POINTER(C.c_int32)), ("kf_pose", C.c_void_p), ("mp_pos", C.c_void_p),
                ("max_kf_rows", C.c_int), ("max_pt_rows", C.c_int), ("max_obs", C.c_int)] + \
               [(k, C.c_void_p) for k in ("kf_off", "kf_Tcw", "kf_fixed", "kf_slot", "kf_id", "pt_off", "pt_pos",
                                          "pt_id", "obs_off", "obs_kf", "obs_kp", "counts", "status")]


class LocalBaApply(C.Structure):
    """orbx_local_ba_apply."""
    _fields_ = [("batch", C.c_int), ("max_kf_rows", C.c_int), ("max_pt_rows", C.c_int)] + \
               [(k, C.c_void_p) for k in ("kf_off", "kf_id", "kf_fixed", "kf_Tcw_opt", "pt_off", "pt_id", "pt_pos_opt",
                                          "obs_off", "obs_kf", "obs_kp", "erase")] + \
               [("n_keyframes", C.c_int), ("n_mappoints", C.c_int), ("cap", C.c_int), ("kf_pose", C.c_void_p),
                ("mp_pos", C.c_void_p), ("kf_mp", C.c_void_p)]


ORBX_LOCAL_MAP_STATUS_CAPACITY = 1
ORBX_LOCAL_MAP_STATUS_EMPTY = 2


class LocalMapUpdate(C.Structure):
    """orbx_local_map_update."""
    _fields_ = [("batch", C.c_int), ("cap", C.c_int), ("frame_mp", C.c_void_p), ("n", C.c_void_p), ("parent", C.c_void_p),
                ("max_local_kf", C.c_int), ("max_local_points", C.c_int), ("max_total", C.c_int)] + \
               [(k, C.c_void_p) for k in ("local_kf", "local_kf_n", "ref_kf", "local_off", "local_ids", "counts", "status")]


class TrackLocalMapTally(C.Structure):
    """orbx_track_local_map_tally."""
    _fields_ = [("batch", C.c_int), ("cap", C.c_int), ("frame_mp", C.c_void_p), ("n", C.c_void_p), ("outlier", C.c_void_p),
                ("n_mappoints", C.c_int), ("observations", C.c_void_p), ("only_tracking", C.c_int), ("stereo", C.c_int),
                ("recently_relocalised", C.c_void_p), ("mp_found", C.c_void_p), ("matches_inliers", C.c_void_p),
                ("ok", C.c_void_p)]


ORBX_CULL_STATUS_NO_PARENT = 1


class MapTables(C.Structure):
    """orbx_map_tables."""
    _fields_ = [(k, C.c_void_p) for k in ("kf_mp", "kf_bad", "mp_bad", "kf_keys_un", "kf_u_right", "kf_depth",
                                          "kf_th_depth", "kf_not_erase", "kf_to_be_erased")]


ORBX_NORMAL_STATUS_REF_NOT_OBSERVER = 1
ORBX_NORMAL_STATUS_BAD_INDEX = 2


class NormalDepth(C.Structure):
    """orbx_normal_depth."""
    _fields_ = [("kf_Tcw", C.c_void_p), ("kf_keys_un", C.c_void_p), ("mp_ref_kf", C.c_void_p), ("mp_pos", C.c_void_p),
                ("scale_factors", C.POINTER(C.c_float)), ("nlevels", C.c_int), ("normal", C.c_void_p),
                ("max_distance", C.c_void_p), ("min_distance", C.c_void_p)]


class CorrectLoopPropagate(C.Structure):
    """orbx_correct_loop_propagate."""
    _fields_ = [("cur_kf", C.c_int), ("Scw", C.c_void_p), ("sim3_R", C.c_void_p), ("sim3_t", C.c_void_p),
                ("sim3_s", C.c_void_p), ("matched_kf", C.c_int), ("kf_Tcw", C.c_void_p), ("mp_pos", C.c_void_p),
                ("mp_corrected_by_kf", C.c_void_p), ("mp_corrected_ref", C.c_void_p), ("mp_ref_kf", C.c_void_p),
                ("kf_keys_un", C.c_void_p), ("scale_factors", C.POINTER(C.c_float)), ("nlevels", C.c_int),
                ("normal", C.c_void_p), ("max_distance", C.c_void_p), ("min_distance", C.c_void_p), ("conn", C.c_void_p),
                ("n_conn", C.c_void_p), ("corr_S", C.c_void_p), ("kf_corr", C.c_void_p), ("kf_Tcw_nc", C.c_void_p),
                ("status", C.c_void_p)]


ORBX_ASSEMBLY_STATUS_CAPACITY = 1
ORBX_ASSEMBLY_STATUS_BAD_KEYFRAME = 2


class EssentialGraphAssembly(C.Structure):
    """orbx_essential_graph_assembly."""
    _fields_ = ([("cur_kf", C.c_int), ("loop_kf", C.c_int), ("min_feat", C.c_int)] +
                [(k, C.c_void_p) for k in ("conn", "n_conn", "kf_corr", "kf_Tcw_nc", "kf_Tcw", "loop_off", "loop_kf_ids",
                                           "mp_corrected_by_kf", "mp_corrected_ref", "mp_ref_kf")] +
                [("max_lc", C.c_int), ("max_edges", C.c_int)] +
                [(k, C.c_void_p) for k in ("lc_off", "lc_member", "lc_kf", "lc_w", "kf_ids", "kf_row", "n_rows", "kf_off",
                                           "loop_row", "kf_corr_rows", "kf_Tcw_rows", "edge_v", "edge_kind", "n_edges",
                                           "edge_off", "pt_ref", "pt_off", "env_blocks", "status")])


# ---- handle lifetime (DESIGN.md §1 "Teardown") ------------------------------------
# Every object that owns liborbx handles or HIP streams registers here.  At interpreter
# exit the atexit hook synchronises the devices and closes them newest first -- while the
# HIP runtime, RCCL and any profiler are still fully alive -- so no HIP object is left for
# the C runtime's static destructors (HIP's own, RCCL's, a profiler tool's) to tear down in
# whatever order they run.  __del__ does nothing once the interpreter is finalizing.
_handles: list = []
_hook = False


def track(obj) -> None:
    """Register a handle owner (it has close(): idempotent, synchronising what it frees)."""
    global _hook
    import weakref
    if len(_handles) > 4096:  # drop the owners already freed
        _handles[:] = [r for r in _handles if r() is not None]
    _handles.append(weakref.ref(obj))
    if not _hook:
        # registered after torch's own exit hooks (lib() imports torch first), so it runs
        # before them
        import atexit
        atexit.register(release_all)
        _hook = True


def release_all() -> int:
    """Synchronise the devices the process used and close every live handle owner,
    newest first; returns how many were closed."""
    live = [o for o in (r() for r in reversed(_handles)) if o is not None]
    _handles.clear()
    if not live:
        return 0
    try:
        import torch
        if torch.cuda.is_initialized():
            for d in range(torch.cuda.device_count()):
                with torch.cuda.device(d):
                    torch.cuda.synchronize()
    except Exception:
        pass
    for o in live:
        try:
            o.close()
        except Exception:
            pass
    return len(live)


class OrbxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"orbx error {code}: {msg}")
        self.code = code


_lib = None


def lib() -> C.CDLL:
    """Load liborbx.so (raises if it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} not built: run `python -m orbslam2commentedbyxcm_amd.build`")
    # torch bundles its own libamdhip64.so.7 (and HSA runtime).  Two HIP runtimes in one
    # process cannot both open the GPU, so when torch is installed it is loaded first and
    # liborbx.so binds to the same runtime (same SONAME); without torch liborbx.so uses
    # the system ROCm runtime.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(str(LIB_PATH))
    vp, ip, u8p = C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    fp = C.POINTER(C.c_float)
    L.orbx_extractor_create.argtypes = [C.POINTER(ExtractorParams), C.c_int, C.POINTER(vp)]
    L.orbx_extractor_destroy.argtypes = [vp]
    L.orbx_extractor_destroy.restype = None
    L.orbx_extractor_levels.argtypes = [vp, ip, fp, fp, fp, fp]
    L.orbx_extractor_features_per_level.argtypes = [vp, ip]
    L.orbx_extractor_max_keypoints.argtypes = [vp, C.c_int, C.c_int, ip]
    L.orbx_extract.argtypes = [vp, u8p, C.c_int, C.c_int, C.c_size_t, vp, u8p, C.c_int, ip]
    L.orbx_extract_batch.argtypes = [vp, C.c_int, C.POINTER(u8p), C.c_int, C.c_int, C.c_size_t, vp, u8p,
                                     C.c_int, ip]
    L.orbx_extract_batch_device.argtypes = [vp, C.c_int, vp, C.c_size_t, C.c_int, C.c_int, C.c_size_t, vp, vp,
                                            C.c_int, vp, vp]
    L.orbx_extractor_stream.argtypes = [vp]
    L.orbx_extractor_stream.restype = vp
    L.orbx_extractor_set_stage_event.argtypes = [vp, C.c_int, C.POINTER(vp)]
    L.orbx_stream_wait_event.argtypes = [vp, vp]
    L.orbx_stream_create.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.orbx_stream_destroy.argtypes = [vp]
    L.orbx_extractor_status.argtypes = [vp, C.c_int, ip, ip]
    L.orbx_extractor_status_device.argtypes = [vp, C.POINTER(vp)]
    L.orbx_extractor_set_node_capacity.argtypes = [vp, C.c_int]
    L.orbx_extractor_set_level0_in_place.argtypes = [vp, C.c_int]
    L.orbx_extractor_set_timing.argtypes = [vp, C.c_int]
    L.orbx_extractor_stage_times.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), fp, ip]
    L.orbx_pyramid_level.argtypes = [vp, C.c_int, C.c_int, u8p, C.c_size_t, ip, ip]
    L.orbx_pyramid_level_device.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp), C.POINTER(C.c_size_t), ip, ip]
    L.orbx_hamming.argtypes = [u8p, u8p]
    L.orbx_hamming_matrix_device.argtypes = [vp, C.c_int, vp, C.c_int, vp, vp]
    L.orbx_window_match_device.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp]
    i32p = C.POINTER(C.c_int32)
    L.orbx_window_match.argtypes = [C.c_int, u8p, C.c_int, u8p, C.c_int, i32p, i32p, i32p, C.c_int, i32p, i32p,
                                    i32p, i32p, i32p]
    L.orbx_matcher_create.argtypes = [C.c_int, C.c_float, C.c_int, C.POINTER(vp)]
    L.orbx_matcher_destroy.argtypes = [vp]
    L.orbx_matcher_destroy.restype = None
    L.orbx_search_by_projection_local.argtypes = [vp, vp, i32p, i32p, C.c_int, vp, vp, C.c_float, ip]
    L.orbx_search_by_projection_frame.argtypes = [vp, vp, i32p, vp, i32p, u8p, vp, C.c_float, C.c_int, ip]
    L.orbx_search_for_triangulation.argtypes = [vp, vp, u8p, i32p, i32p, i32p, C.c_int, vp, u8p, i32p, i32p, i32p,
                                                C.c_int, fp, C.c_int, i32p, ip]
    L.orbx_compute_stereo_matches.argtypes = [vp, vp, C.c_int, vp, C.c_int, vp, vp, u8p, C.c_int, C.c_float, fp, fp]
    L.orbx_compute_stereo_matches_batch_device.argtypes = [vp, vp, C.c_int, vp, C.c_int, C.c_int, vp, vp, vp, vp, vp,
                                                           vp, C.c_int, C.c_float, C.c_float, vp, vp, vp]
    L.orbx_search_for_triangulation_batch_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, i32p, fp, C.c_int,
                                                             C.c_int, vp, vp, vp, vp]
    L.orbx_match_sequence_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_float, C.c_float, C.c_float,
                                             C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, fp, C.c_int,
                                             C.c_float, C.c_float, vp, vp, vp]
    L.orbx_match_sequence_device_ex.argtypes = [vp, C.POINTER(Sequence), vp]
    L.orbx_search_local_points_device.argtypes = [vp, C.POINTER(MapPointsDevice), C.POINTER(LocalMapBatch), vp]
    L.orbx_create_mappoints_device.argtypes = [C.c_int, vp, vp, C.c_int, vp, C.c_float, vp, C.c_float, C.c_float,
                                               C.c_float, C.c_float, fp, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_update_last_frame_device.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp, C.c_float, C.c_float, C.c_float,
                                                C.c_float, C.c_float, vp, vp, vp, vp, vp, vp]
    L.orbx_search_by_projection_keyframe.argtypes = [vp, vp, i32p, vp, i32p, u8p, vp, C.c_float, C.c_int, ip]
    L.orbx_search_by_projection_sim3.argtypes = [vp, vp, fp, i32p, C.c_int, i32p, vp, C.c_int, ip]
    L.orbx_search_by_bow_frame.argtypes = [vp, vp, i32p, i32p, i32p, i32p, C.c_int, vp, i32p, i32p, i32p, C.c_int,
                                           i32p, ip]
    L.orbx_search_by_bow_keyframes.argtypes = [vp, vp, i32p, i32p, i32p, i32p, C.c_int, vp, i32p, i32p, i32p, i32p,
                                               C.c_int, i32p, ip]
    L.orbx_search_for_initialization.argtypes = [vp, vp, vp, fp, i32p, C.c_int, ip]
    cp = C.POINTER(Camera)
    L.orbx_undistort_keypoints.argtypes = [C.c_int, cp, vp, C.c_int, vp]
    L.orbx_undistort_keypoints_device.argtypes = [cp, C.c_int, vp, vp, C.c_int, vp, vp]
    L.orbx_compute_image_bounds.argtypes = [C.c_int, cp, C.c_int, C.c_int, fp]
    L.orbx_compute_stereo_from_rgbd_device.argtypes = [cp, C.POINTER(RgbdBatch), vp]
    L.orbx_compute_stereo_from_rgbd.argtypes = [C.c_int, cp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_size_t,
                                                C.c_float, C.c_float, vp, fp, fp]
    L.orbx_assign_features_to_grid.argtypes = [C.c_int, vp, C.c_int, fp, i32p, i32p]
    L.orbx_assign_features_to_grid_device.argtypes = [C.c_int, vp, vp, C.c_int, fp, vp, vp, vp]
    L.orbx_fuse.argtypes = [vp, vp, i32p, C.c_int, u8p, vp, C.c_float, i32p]
    L.orbx_fuse_sim3.argtypes = [vp, vp, fp, i32p, C.c_int, u8p, vp, C.c_float, i32p]
    L.orbx_search_by_sim3.argtypes = [vp, vp, i32p, u8p, vp, i32p, u8p, vp, C.c_float, fp, fp, C.c_float, i32p, ip]
    L.orbx_compute_distinctive_descriptors.argtypes = [C.c_int, C.c_int, i32p, u8p, i32p, u8p]
    L.orbx_compute_distinctive_descriptors_device.argtypes = [C.c_int, vp, vp, vp, vp, vp]
    L.orbx_matcher_set_timing.argtypes = [vp, C.c_int]
    L.orbx_matcher_set_footprint.argtypes = [vp, C.c_int]
    L.orbx_matcher_last_ms.argtypes = [vp, fp]
    L.orbx_matcher_last_call_us.argtypes = [vp]
    L.orbx_matcher_last_call_us.restype = C.c_double
    L.orbx_extractor_last_call_us.argtypes = [vp]
    L.orbx_extractor_last_call_us.restype = C.c_double
    dp = C.POINTER(C.c_double)
    L.orbx_vocabulary_load_text_file.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.orbx_vocabulary_load_text.argtypes = [C.c_char_p, C.c_size_t, C.c_int, C.POINTER(vp)]
    L.orbx_vocabulary_destroy.argtypes = [vp]
    L.orbx_vocabulary_destroy.restype = None
    L.orbx_vocabulary_info.argtypes = [vp, ip, ip, ip, ip, ip, ip]
    L.orbx_vocabulary_stream.argtypes = [vp]
    L.orbx_vocabulary_stream.restype = vp
    L.orbx_vocabulary_transform_features.argtypes = [vp, u8p, C.c_int, C.c_int, i32p, dp, i32p]
    L.orbx_vocabulary_transform.argtypes = [vp, u8p, C.c_int, C.c_int, i32p, dp, ip, i32p, i32p, i32p, ip]
    L.orbx_vocabulary_transform_batch_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, C.c_int] + [vp] * 9 + [vp]
    L.orbx_vocabulary_set_timing.argtypes = [vp, C.c_int]
    L.orbx_vocabulary_stage_times.argtypes = [vp, fp, fp]
    L.orbx_debug_set.argtypes = [C.c_char_p, C.c_int]
    L.orbx_bow_score.argtypes = [i32p, dp, C.c_int, i32p, dp, C.c_int, dp]
    L.orbx_kfdb_create.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.orbx_kfdb_destroy.argtypes = [vp]
    L.orbx_kfdb_destroy.restype = None
    L.orbx_kfdb_info.argtypes = [vp, ip, ip, ip]
    L.orbx_kfdb_stream.argtypes = [vp]
    L.orbx_kfdb_stream.restype = vp
    L.orbx_kfdb_add_batch_device.argtypes = [vp, C.c_int, i32p, vp, vp, vp, C.c_int, vp]
    L.orbx_kfdb_add.argtypes = [vp, C.c_int, i32p, dp, C.c_int]
    L.orbx_kfdb_erase.argtypes = [vp, C.c_int]
    L.orbx_kfdb_clear.argtypes = [vp]
    L.orbx_kfdb_set_covisibility.argtypes = [vp, C.c_int, i32p, C.c_int]
    L.orbx_kfdb_reloc_scores.argtypes = [vp, fp]
    L.orbx_kfdb_score_device.argtypes = [vp, vp, vp, vp, C.c_int, vp, C.c_int, vp, vp]
    L.orbx_kfdb_detect_relocalization_candidates_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, C.c_int, vp,
                                                                    vp, vp, vp]
    L.orbx_kfdb_detect_loop_candidates_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int,
                                                          vp, vp, vp, vp]
    L.orbx_kfdb_detect_relocalization_candidates.argtypes = [vp, i32p, dp, C.c_int, i32p, C.c_int, ip]
    L.orbx_kfdb_detect_loop_candidates.argtypes = [vp, i32p, dp, C.c_int, i32p, C.c_int, C.c_float, i32p, C.c_int, ip]
    L.orbx_pose_optimization_batch_device.argtypes = [vp, C.POINTER(PoseOptimizationBatch), vp]
    L.orbx_pose_optimization.argtypes = [vp, vp, C.c_int, fp, i32p, fp, C.c_int, fp, C.c_int, C.c_float, C.c_float,
                                         C.c_float, C.c_float, C.c_float, fp, fp, u8p, ip, i32p, ip]
    L.orbx_sim3_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.orbx_sim3_destroy.argtypes = [vp]
    L.orbx_sim3_destroy.restype = None
    L.orbx_sim3_set_batch_device.argtypes = [vp, C.POINTER(Sim3Batch), vp]
    L.orbx_sim3_iterate_device.argtypes = [vp, C.c_int, C.POINTER(Sim3Result), vp]
    L.orbx_sim3_set.argtypes = [vp, C.POINTER(Sim3Batch)]
    L.orbx_sim3_iterate.argtypes = [vp, C.c_int, C.POINTER(Sim3Result)]
    L.orbx_sim3_draws.argtypes = [i32p, C.c_int, C.c_int]
    L.orbx_pnp_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.orbx_pnp_destroy.argtypes = [vp]
    L.orbx_pnp_destroy.restype = None
    L.orbx_pnp_set_batch_device.argtypes = [vp, C.POINTER(PnpBatch), vp]
    L.orbx_pnp_iterate_device.argtypes = [vp, C.c_int, C.POINTER(PnpResult), vp]
    L.orbx_pnp_set.argtypes = [vp, C.POINTER(PnpBatch)]
    L.orbx_pnp_iterate.argtypes = [vp, C.c_int, C.POINTER(PnpResult)]
    L.orbx_pnp_draws.argtypes = [i32p, C.c_int, C.c_int]
    L.orbx_optimize_sim3_batch_device.argtypes = [vp, C.POINTER(OptimizeSim3Batch), vp]
    L.orbx_optimize_sim3.argtypes = [vp, C.POINTER(OptimizeSim3Batch)]
    L.orbx_local_bundle_adjustment_batch_device.argtypes = [vp, C.POINTER(LocalBaBatch), vp]
    L.orbx_local_bundle_adjustment.argtypes = [vp, C.POINTER(LocalBaBatch)]
    L.orbx_global_bundle_adjustment_batch_device.argtypes = [vp, C.POINTER(GlobalBaBatch), vp]
    L.orbx_global_bundle_adjustment.argtypes = [vp, C.POINTER(GlobalBaBatch)]
    L.orbx_global_ba_envelope.argtypes = [C.c_int, vp, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int64)]
    L.orbx_optimize_essential_graph_batch_device.argtypes = [vp, C.POINTER(EssentialGraphBatch), vp]
    L.orbx_optimize_essential_graph.argtypes = [vp, C.POINTER(EssentialGraphBatch)]
    L.orbx_essential_graph_envelope.argtypes = [C.c_int, C.c_int, vp, C.c_int, C.POINTER(C.c_int64)]
    L.orbx_triangulate_pairs_batch_device.argtypes = [vp, C.c_int, vp, vp, C.c_int, i32p, C.c_int, vp, vp, C.c_float,
                                                      C.c_float, C.POINTER(NewMapPoints), vp]
    L.orbx_triangulate_pairs.argtypes = [vp, C.POINTER(KeyFrameGeomDevice), C.POINTER(KeyFrameGeomDevice), vp, C.c_int,
                                         i32p, C.c_float, C.c_float, C.POINTER(NewMapPoints)]
    L.orbx_initializer_create.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.orbx_initializer_destroy.argtypes = [vp]
    L.orbx_initializer_destroy.restype = None
    L.orbx_initializer_initialize_device.argtypes = [vp, C.POINTER(InitializerBatch), C.POINTER(InitializerResult), vp]
    L.orbx_initializer_initialize.argtypes = [vp, C.POINTER(InitializerBatch), C.POINTER(InitializerResult)]
    L.orbx_initializer_sets.argtypes = [i32p, C.c_int, C.c_int]
    L.orbx_covis_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.orbx_covis_destroy.argtypes = [vp]
    L.orbx_covis_destroy.restype = None
    L.orbx_covis_stream.argtypes = [vp]
    L.orbx_covis_stream.restype = vp
    L.orbx_covis_refresh_observations_device.argtypes = [vp, C.c_int, vp, vp, vp, C.c_int, vp, vp]
    L.orbx_covis_refresh_observations.argtypes = [vp, C.c_int, i32p, i32p, u8p, C.c_int, u8p]
    L.orbx_covis_update_connections_device.argtypes = [vp, i32p, C.c_int, vp]
    L.orbx_covis_erase_keyframe_device.argtypes = [vp, C.c_int, vp]
    L.orbx_covis_view_device.argtypes = [vp, C.POINTER(CovisView)]
    L.orbx_covis_best_covisibles_device.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbx_covis_covisibles_by_weight_device.argtypes = [vp, C.c_int, vp, vp, vp]
    L.orbx_local_ba_assemble_device.argtypes = [vp, C.POINTER(LocalBaAssembly), vp]
    L.orbx_local_ba_apply_device.argtypes = [vp, C.POINTER(LocalBaApply), vp]
    L.orbx_covis_read.argtypes = [vp, vp, vp, C.c_size_t]
    L.orbx_update_local_map_device.argtypes = [vp, C.POINTER(LocalMapUpdate), vp]
    L.orbx_update_local_map.argtypes = [vp, C.POINTER(LocalMapUpdate)]
    L.orbx_search_local_points_offsets_device.argtypes = [vp, C.POINTER(MapPointsDevice), C.POINTER(LocalMapBatch), vp,
                                                          C.c_int, C.c_int, vp]
    L.orbx_track_local_map_tally_device.argtypes = [vp, C.POINTER(TrackLocalMapTally), vp]
    L.orbx_covis_ordered.argtypes = [vp, C.c_int, i32p, i32p, C.c_int, ip]
    L.orbx_keyframe_culling_device.argtypes = [vp, C.POINTER(MapTables), C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]
    L.orbx_covis_set_bad_flag_device.argtypes = [vp, C.POINTER(MapTables), i32p, C.c_int, vp, vp, vp]
    L.orbx_map_point_culling_device.argtypes = [vp, C.POINTER(MapTables), C.c_int, C.c_int, vp, vp, C.c_int, vp, vp, vp,
                                                vp, vp]
    L.orbx_covis_observation_counts_device.argtypes = [vp, vp, vp, vp]
    L.orbx_update_normal_and_depth_device.argtypes = [vp, C.POINTER(NormalDepth), vp, C.c_int, vp, vp]
    L.orbx_correct_loop_propagate_device.argtypes = [vp, C.POINTER(CorrectLoopPropagate), vp]
    L.orbx_essential_graph_assemble_device.argtypes = [vp, C.POINTER(EssentialGraphAssembly), vp]
    L.orbx_version.restype = C.c_char_p
    L.orbx_device_count.argtypes = [ip]
    L.orbx_last_error.restype = C.c_char_p
    _lib = L
    return L


def debug_set(name: str | None, value: int = -1) -> None:
    """orbx_debug_set: select an alternative kernel form or a diagnostics switch
    (value < 0: the default; name None: every default).  Tests and A/B tools only."""
    check(lib().orbx_debug_set(None if name is None else name.encode(), int(value)))


def check(rc: int, allow=(ORBX_OK,)) -> int:
    if rc in allow:
        return rc
    msg = lib().orbx_last_error().decode(errors="replace")
    raise OrbxError(rc, msg)


def u8ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def i32ptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))
