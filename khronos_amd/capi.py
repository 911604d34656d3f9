"""ctypes binding of the C ABI in include/khronos_amd.h (plumbing only: the product is the HIP library).

Fails loudly when the HIP extension is missing: there is no CPU fallback for the fusion path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libkhronos_amd.so")

KHR_OK, KHR_EINVAL, KHR_ENOMEM, KHR_EDEVICE, KHR_ENOTFOUND, KHR_ESTATE = 0, -1, -2, -3, -4, -5
VOX_ACTIVE, VOX_EVER_FREE, VOX_TO_REMOVE, VOX_SEM_VALID = 1, 2, 4, 8
BLK_UPDATED, BLK_MESH_UPDATED, BLK_TRACKING_UPDATED, BLK_HAS_ACTIVE_DATA = 1, 2, 4, 8


class KhrConfig(C.Structure):
    _fields_ = [
        ("voxel_size", C.c_float), ("voxels_per_side", C.c_int32), ("truncation_distance", C.c_float),
        ("with_semantics", C.c_int32), ("with_tracking", C.c_int32), ("num_labels", C.c_int32),
        ("use_weight_dropoff", C.c_int32), ("weight_dropoff_epsilon", C.c_float),
        ("use_constant_weight", C.c_int32), ("max_weight", C.c_float), ("interpolation_method", C.c_int32),
        ("adaptive_max_range_difference", C.c_float), ("range_mode", C.c_int32), ("semantic_mode", C.c_int32),
        ("label_confidence", C.c_float),
        ("temporal_buffer", C.c_float), ("tsdf_occupancy_threshold", C.c_float),
        ("neighbor_connectivity", C.c_int32), ("temporal_window", C.c_float),
        ("md_neighbor_connectivity", C.c_int32), ("md_min_cluster_size", C.c_int32),
        ("md_max_cluster_size", C.c_int32), ("md_min_separation_distance", C.c_float),
        ("md_max_range", C.c_float), ("md_min_z_coordinate", C.c_float),
        ("mesh_min_weight", C.c_float),
        ("max_blocks", C.c_uint32), ("max_frame_pixels", C.c_uint32), ("num_frame_slots", C.c_uint32),
        ("max_mesh_vertices", C.c_uint64), ("max_band_records", C.c_uint32), ("disable_culling", C.c_int32),
        ("device", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32), ("relaxed_arithmetic", C.c_int32), ("max_snapshot_blocks", C.c_uint32),
        ("alloc_candidate", C.c_int32), ("color_blend_weight", C.c_int32), ("mesh_attr_source", C.c_int32), ("mesh_degenerate_eps", C.c_float),
        ("packed_likelihood_rows", C.c_int32),
    ]


class KhrSensor(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_float), ("fy", C.c_float),
                ("cx", C.c_float), ("cy", C.c_float), ("min_range", C.c_float), ("max_range", C.c_float)]


class KhrRenderRequest(C.Structure):
    _fields_ = [("sensor", KhrSensor), ("world_T_sensor", C.c_double * 16), ("step_voxels", C.c_float), ("min_weight", C.c_float)]


class KhrRenderStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_hit", "n_blocked", "n_samples_total", "n_samples_evaluated")]


class KhrQueryStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_value", "n_gradient", "n_voxel")]


KHR_QP_VALUE, KHR_QP_GRADIENT, KHR_QP_VOXEL = 1, 2, 4


class KhrWeldStats(C.Structure):
    _fields_ = [("n_soup_vertices", C.c_uint64), ("n_vertices", C.c_uint64), ("n_faces", C.c_uint64), ("n_degenerate_faces", C.c_uint64)]


KHR_MERGE_ALIGNED, KHR_MERGE_RESAMPLE = 0, 1


class KhrMergeRequest(C.Structure):
    _fields_ = [("mode", C.c_int32), ("voxel_offset", C.c_int32 * 3), ("dst_T_src", C.c_double * 16), ("min_weight", C.c_float)]


class KhrMergeStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_src_blocks", "n_candidate_blocks", "n_touched_blocks", "n_new_blocks", "n_added_voxels",
                                          "n_merged_voxels")]


KHR_DIFF_APPEARED, KHR_DIFF_DISAPPEARED = 1, 2


class KhrDiffRequest(C.Structure):
    _fields_ = [("mode", C.c_int32), ("voxel_offset", C.c_int32 * 3), ("ctx_T_ref", C.c_double * 16), ("min_weight", C.c_float),
                ("occupied_distance", C.c_float), ("free_distance", C.c_float)]


class KhrDiffStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_ref_blocks", "n_candidate_blocks", "n_present_blocks", "n_compared_voxels", "n_appeared",
                                          "n_disappeared", "n_only_now", "n_only_then", "n_changed_blocks")]


class KhrSegmentRequest(C.Structure):
    _fields_ = [("min_weight", C.c_float), ("surface_distance", C.c_float), ("connectivity", C.c_int32), ("by_label", C.c_int32),
                ("labels", C.POINTER(C.c_int32)), ("n_labels", C.c_int32), ("flags_require", C.c_uint32), ("flags_exclude", C.c_uint32),
                ("min_voxels", C.c_int64), ("max_voxels", C.c_int64), ("want_voxels", C.c_int32)]


class KhrSegmentStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_blocks", "n_member_voxels", "n_components_all", "n_too_small", "n_too_large", "n_components",
                                          "n_voxels")]


class KhrDfRequest(C.Structure):
    _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("ratio", C.c_int32), ("min_weight", C.c_float),
                ("max_distance", C.c_float), ("surface_distance", C.c_float), ("unknown_is_obstacle", C.c_int32),
                ("positive_only", C.c_int32)]


class KhrDfStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_observed", "n_obstacle", "n_free", "n_in_range")]


KHR_DF_OBSERVED, KHR_DF_OBSTACLE, KHR_DF_IN_RANGE = 1, 2, 4
KHR_DF_MAX_DIM, KHR_DF_FAR = 512, 1 << 30


class KhrVoronoiRequest(C.Structure):
    _fields_ = [("origin", C.c_int32 * 3), ("dims", C.c_int32 * 3), ("ratio", C.c_int32), ("min_weight", C.c_float),
                ("max_distance", C.c_float), ("surface_distance", C.c_float), ("unknown_is_obstacle", C.c_int32),
                ("min_distance", C.c_float), ("mode", C.c_int32), ("parent_l1_separation", C.c_int32),
                ("parent_cos_angle_separation", C.c_float), ("min_basis", C.c_int32)]


class KhrVoronoiStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_observed", "n_obstacle", "n_free", "n_in_range", "n_eligible", "n_basis2", "n_basis3",
                                          "n_basis4", "n_listed")]


KHR_VOR_L1, KHR_VOR_ANGLE, KHR_VOR_L1_THEN_ANGLE, KHR_VOR_MAX_BASIS = 0, 1, 2, 4


class KhrPlacesRequest(C.Structure):
    _fields_ = [("min_basis", C.c_int32), ("min_node_distance", C.c_float), ("compression", C.c_int32), ("min_component_size", C.c_int32)]


class KhrPlacesStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_members", "n_places_all", "n_edges_all", "n_components_all", "n_places", "n_edges", "n_components")]


KHR_PL_MAX_COMPRESSION = 16


class KhrTravelRequest(C.Structure):
    _fields_ = [("clearance", C.c_float), ("connectivity", C.c_int32), ("allow_unknown", C.c_int32), ("max_cost", C.c_uint32)]


class KhrTravelStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_traversable", "n_goals_used", "n_reached", "max_cost", "n_rounds", "n_waits")]


KHR_TF_UNREACHED, KHR_TF_TILE_EDGE, KHR_TF_ROUNDS_PER_WAIT = 0xFFFFFFFF, 8, 8


class KhrAlignRequest(C.Structure):
    _fields_ = [("n", C.c_int64), ("points", C.c_void_p), ("depth", C.c_void_p), ("sensor", KhrSensor), ("stride", C.c_int32),
                ("weights", C.c_void_p), ("world_T_source", C.c_double * 16), ("min_weight", C.c_float), ("gate", C.c_float),
                ("huber_delta", C.c_float)]


class KhrAlignOptions(C.Structure):
    _fields_ = [("max_iterations", C.c_int32), ("min_inliers", C.c_int32), ("lambda_", C.c_double), ("eps_rot", C.c_double),
                ("eps_trans", C.c_double)]


class KhrAlignResult(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32), ("n_inlier_first", C.c_uint64), ("n_inlier_last", C.c_uint64),
                ("rmse_first", C.c_double), ("rmse_last", C.c_double), ("H", C.c_double * 21), ("b", C.c_double * 6)]


KHR_ALIGN_WORDS, KHR_ALIGN_MAX_SOURCES = 32, 1 << 20


class KhrFrame(C.Structure):
    _fields_ = [("timestamp_ns", C.c_uint64), ("world_T_sensor", C.c_double * 16), ("depth", C.c_void_p),
                ("color", C.c_void_p), ("label", C.c_void_p)]


class KhrConvertedFrame(C.Structure):
    _fields_ = [("timestamp_ns", C.c_uint64), ("world_T_sensor", C.c_double * 16), ("range", C.c_void_p), ("depth", C.c_void_p),
                ("rgba", C.c_void_p), ("label", C.c_void_p), ("tile_max", C.c_void_p)]


class KhrCluster(C.Structure):
    _fields_ = [("id", C.c_int32), ("num_pixels_listed", C.c_uint64), ("num_pixels_painted", C.c_uint32),
                ("bbox_min", C.c_float * 3), ("bbox_max", C.c_float * 3), ("centroid", C.c_float * 3),
                ("semantic_id", C.c_int32)]


class KhrObjectDetectorConfig(C.Structure):
    _fields_ = [("use_full_connectivity", C.c_int32), ("min_cluster_size", C.c_int32), ("max_cluster_size", C.c_int32),
                ("use_3d", C.c_int32), ("grid_size", C.c_float), ("max_range", C.c_float),
                ("object_labels", C.POINTER(C.c_int32)), ("n_object_labels", C.c_int32)]


CKPT_SECTIONS = ("indices", "distance", "weight", "color", "last_observed", "last_occupied", "flags", "sem_label", "block_flags",
                 "likelihoods")


class KhrCheckpointHeader(C.Structure):
    _fields_ = [("magic", C.c_uint32), ("version", C.c_uint32), ("voxel_size", C.c_float), ("voxels_per_side", C.c_int32),
                ("truncation_distance", C.c_float), ("with_semantics", C.c_int32), ("with_tracking", C.c_int32),
                ("num_labels", C.c_int32), ("semantic_mode", C.c_int32), ("header_bytes", C.c_uint32),
                ("num_blocks", C.c_uint64), ("total_bytes", C.c_uint64), ("offset", C.c_uint64 * len(CKPT_SECTIONS))]


class KhrStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "n_allocated_blocks", "n_visible_blocks", "n_new_blocks", "n_visited_voxels", "n_updated_voxels",
        "n_band_voxels", "n_tracking_updated_blocks", "n_seeds", "n_mesh_blocks", "n_mesh_vertices",
        "pool_exhausted", "cum_updated_voxels", "cum_band_voxels", "cum_visited_voxels", "cum_integrate_calls", "n_tsdf_blocks", "band_overflow",
        "n_tracking_processed_blocks", "n_fuse_items", "n_seed_waits", "n_seed_waits_late", "seed_wait_max_us")] + [
        ("seed_wait_hist", C.c_uint64 * 8)] + [(n, C.c_uint64) for n in (
        "seed_wait_late_us", "seed_wait_late_frame", "seed_wait_late_state", "n_md_device_merges", "n_md_host_walks",
        "n_md_prelaunched", "n_md_prelaunch_repeats")]


# every symbol include/khronos_amd.h declares (tests check the library exports all of them)
EXPORTS = [
    "khr_create", "khr_destroy", "khr_last_error", "khr_host_trace", "khr_set_stream", "khr_sync", "khr_default_config",
    "khr_upload_frame", "khr_set_frame_image", "khr_download_frame", "khr_frame_copy_create", "khr_frame_copy_download", "khr_frame_copy_release", "khr_integrate", "khr_update_tracking",
    "khr_detect_motion", "khr_generate_mesh", "khr_reset_inactive", "khr_mark_all_inactive", "khr_clear_updated",
    "khr_allocate_blocks", "khr_object_prune", "khr_begin_object_map", "khr_integrate_prune_batch", "khr_get_stats", "khr_num_blocks", "khr_block_indices",
    "khr_download_block", "khr_mesh_num_vertices", "khr_download_mesh", "khr_fetch_mesh", "khr_fetch_mesh_into", "khr_timing_enable", "khr_timing_reset",
    "khr_timing_get", "khr_debug_read", "khr_tick_ingest", "khr_tick_integrate", "khr_tick_live_bound", "khr_tick_seed_counts", "khr_converted_bytes", "khr_export_converted",
    "khr_converted_views", "khr_tick_adopt", "khr_copy_frame_image", "khr_rv_detect_changes", "khr_last_removed", "khr_process_frame", "khr_ingest_ahead", "khr_ingest_ahead_host", "khr_ingest_cancel", "khr_integrate_shared", "khr_integrate_shared_batch", "khr_pixel_iou", "khr_forward_instances", "khr_update_tracking_phase",
    "khr_export_halo", "khr_import_halo", "khr_get_dynamic_clusters", "khr_motion_keys", "khr_motion_bits_bytes", "khr_motion_bits", "khr_detect_motion_from_bits",
    "khr_dynamic_pack_bytes", "khr_dynamic_unpack_bytes",
    "khr_detect_motion_from_keys", "khr_download_updated", "khr_mesh_halo_requests", "khr_mesh_halo_export",
    "khr_mesh_halo_requests_sorted", "khr_mesh_halo_plan", "khr_mesh_halo_answer", "khr_mesh_halo_adopt",
    "khr_mesh_halo_import", "khr_configure_object_detector", "khr_detect_objects", "khr_get_semantic_clusters",
    "khr_cluster_voxels", "khr_download_frame_image", "khr_detect_objects_launch", "khr_pool_exhausted", "khr_map_digest",
    "khr_rv_create", "khr_rv_destroy", "khr_rv_clear", "khr_rv_add_rays", "khr_rv_num_rays", "khr_rv_num_pairs", "khr_rv_check",
    "khr_snapshot_updated", "khr_take_snapshot", "khr_snapshot_num_blocks", "khr_snapshot_download", "khr_snapshot_download_extra", "khr_snapshot_download_begin", "khr_snapshot_download_end", "khr_snapshot_poll", "khr_fetch_mesh_launch", "khr_reserve_mesh_staging", "khr_reserve_snapshots", "khr_mirror_dynamic", "khr_snapshot_release",
    "khr_rv_check_stamps", "khr_get_config", "khr_cluster_voxels_launch", "khr_cluster_voxels_fetch", "khr_reset_map", "khr_depend_on", "khr_retain_slot", "khr_release_slot",
    "khr_map_slice", "khr_slice_voxel_z", "khr_render_view", "khr_query_points",
    "khr_align_linearize", "khr_align_frame", "khr_distance_field",
    "khr_checkpoint_size", "khr_checkpoint_save", "khr_checkpoint_load", "khr_checkpoint_inspect",
    "khr_debug_live_resources", "khr_configure_object_voxel_sets",
    "khr_weld_mesh", "khr_weld_mesh_into", "khr_merge_map", "khr_diff_map", "khr_diff_map_into",
    "khr_segment_map", "khr_segment_map_into", "khr_voronoi_field", "khr_voronoi_field_into",
    "khr_places_graph", "khr_places_graph_from", "khr_places_graph_into", "khr_places_graph_box",
    "khr_travel_field", "khr_travel_field_from", "khr_travel_field_box", "khr_travel_field_into", "khr_travel_paths", "khr_travel_paths_into",
]

_lib = None


class KhronosAmdError(RuntimeError):
    pass


def load_library():
    """Load libkhronos_amd.so (built by __graft_entry__.build()).  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KhronosAmdError(
            "HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'`. "
            "The khronos_amd fusion path has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, u64 = C.c_void_p, C.c_int, C.c_int64, C.c_uint64
    lib.khr_create.argtypes = [C.POINTER(KhrConfig), C.POINTER(vp)]
    lib.khr_create.restype = i32
    lib.khr_destroy.argtypes = [vp]
    lib.khr_destroy.restype = None
    lib.khr_last_error.restype = C.c_char_p
    lib.khr_host_trace.argtypes = [C.c_char_p]
    lib.khr_host_trace.restype = None
    lib.khr_set_stream.argtypes = [vp, vp]
    lib.khr_sync.argtypes = [vp]
    lib.khr_default_config.argtypes = [C.POINTER(KhrConfig)]
    lib.khr_default_config.restype = None
    lib.khr_upload_frame.argtypes = [vp, C.POINTER(KhrSensor), C.POINTER(KhrFrame), i32]
    lib.khr_set_frame_image.argtypes = [vp, i32, i32, vp, i32]
    lib.khr_download_frame.argtypes = [vp, i32, vp, vp, vp]
    lib.khr_integrate.argtypes = [vp, i32, i32, i32, i32]
    lib.khr_integrate_shared.argtypes = [vp, vp, i32, i32, i32, i32]
    lib.khr_integrate_shared_batch.argtypes = [vp, vp, vp, vp, i32, i32, i32]
    lib.khr_update_tracking.argtypes = [vp, u64]
    lib.khr_update_tracking_phase.argtypes = [vp, u64, i32]
    lib.khr_export_halo.argtypes = [vp, vp, i64, i32]
    lib.khr_import_halo.argtypes = [vp, vp, i64, i32]
    lib.khr_detect_motion.argtypes = [vp, i32]
    lib.khr_motion_keys.argtypes = [vp, i32, vp, i32, C.POINTER(C.c_uint32)]
    lib.khr_detect_motion_from_keys.argtypes = [vp, i32, vp, i32]
    lib.khr_get_dynamic_clusters.argtypes = [vp, i32, C.POINTER(KhrCluster), i32]
    lib.khr_configure_object_detector.argtypes = [vp, C.POINTER(KhrObjectDetectorConfig)]
    lib.khr_detect_objects.argtypes = [vp, i32]
    lib.khr_pixel_iou.argtypes = [vp, i32, vp, i32, i32, vp, vp]
    lib.khr_forward_instances.argtypes = [vp, i32, C.c_float, vp, i32, i32, C.POINTER(KhrCluster)]
    lib.khr_download_frame_image.argtypes = [vp, i32, i32, vp]
    lib.khr_rv_create.argtypes = [C.c_float, C.c_float, C.c_float, i32, C.POINTER(vp)]
    lib.khr_rv_destroy.argtypes = [vp]
    lib.khr_rv_destroy.restype = None
    lib.khr_rv_clear.argtypes = [vp]
    lib.khr_rv_add_rays.argtypes = [vp, C.c_int64, vp, vp, vp]
    lib.khr_rv_num_rays.argtypes = [vp]
    lib.khr_rv_num_rays.restype = C.c_int64
    lib.khr_rv_num_pairs.argtypes = [vp]
    lib.khr_rv_num_pairs.restype = C.c_int64
    lib.khr_rv_check.argtypes = [vp, C.c_int64, vp, vp, vp, vp, vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    lib.khr_rv_check_stamps.argtypes = [vp, vp, vp]
    lib.khr_rv_detect_changes.argtypes = [vp, C.c_float, C.c_int64, i32, C.c_float, C.c_float, vp, i32, vp, vp, vp]
    lib.khr_get_config.argtypes = [vp, vp]
    lib.khr_reset_map.argtypes = [vp, C.c_float, C.c_float]
    lib.khr_depend_on.argtypes = [vp, vp]
    lib.khr_retain_slot.argtypes = [vp, i32]
    lib.khr_release_slot.argtypes = [vp, i32]
    lib.khr_cluster_voxels_launch.argtypes = [vp, i32, i32, C.c_float]
    lib.khr_cluster_voxels_fetch.argtypes = [vp, i32, vp, vp, C.c_int64]
    lib.khr_cluster_voxels_fetch.restype = C.c_int64
    lib.khr_configure_object_voxel_sets.argtypes = [vp, C.c_float]
    lib.khr_get_semantic_clusters.argtypes = [vp, i32, C.POINTER(KhrCluster), i32]
    lib.khr_cluster_voxels.argtypes = [vp, i32, i32, C.c_float, vp, vp, C.c_int64]
    lib.khr_cluster_voxels.restype = C.c_int64
    lib.khr_generate_mesh.argtypes = [vp, i32, i32]
    lib.khr_reset_inactive.argtypes = [vp, vp, i64, C.POINTER(i64)]
    lib.khr_mark_all_inactive.argtypes = [vp]
    lib.khr_clear_updated.argtypes = [vp]
    lib.khr_allocate_blocks.argtypes = [vp, vp, i64]
    lib.khr_object_prune.argtypes = [vp, C.c_float, C.c_float, C.POINTER(i64)]
    lib.khr_begin_object_map.argtypes = [vp, C.c_float, C.c_float, vp, vp]
    lib.khr_integrate_prune_batch.argtypes = [vp, vp, vp, vp, i32, i32, C.c_float, C.c_float, C.POINTER(i64)]
    lib.khr_get_stats.argtypes = [vp, C.POINTER(KhrStats)]
    lib.khr_num_blocks.argtypes = [vp]
    lib.khr_num_blocks.restype = i64
    lib.khr_block_indices.argtypes = [vp, vp, i64, i32]
    lib.khr_block_indices.restype = i64
    lib.khr_download_block.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32] + [vp] * 9
    lib.khr_map_slice.argtypes = [vp, i64, i64] + [vp] * 7
    lib.khr_slice_voxel_z.argtypes = [C.c_float, C.c_float, C.c_int32, vp]
    lib.khr_render_view.argtypes = [vp, C.POINTER(KhrRenderRequest), i32] + [vp] * 6 + [C.POINTER(KhrRenderStats)]
    lib.khr_query_points.argtypes = [vp, i64, vp, C.c_float, i32] + [vp] * 8 + [C.POINTER(KhrQueryStats)]
    lib.khr_distance_field.argtypes = [vp, C.POINTER(KhrDfRequest), i32, vp, vp, vp, C.POINTER(KhrDfStats)]
    lib.khr_align_linearize.argtypes = [vp, C.POINTER(KhrAlignRequest), i32, vp]
    lib.khr_align_frame.argtypes = [vp, C.POINTER(KhrAlignRequest), i32, C.POINTER(KhrAlignOptions), vp, C.POINTER(KhrAlignResult)]
    lib.khr_checkpoint_size.argtypes = [vp, C.POINTER(u64), C.POINTER(i64)]
    lib.khr_checkpoint_save.argtypes = [vp, vp, u64, C.POINTER(u64)]
    lib.khr_checkpoint_load.argtypes = [vp, vp, u64, C.POINTER(i64)]
    lib.khr_checkpoint_inspect.argtypes = [vp, u64, C.POINTER(KhrCheckpointHeader)]
    lib.khr_mesh_halo_requests.argtypes = [vp, vp, i64, i32, i32]
    lib.khr_mesh_halo_export.argtypes = [vp, vp, i64, vp, i64, i32]
    lib.khr_mesh_halo_import.argtypes = [vp, vp, i64, i32]
    lib.khr_mesh_halo_requests_sorted.argtypes = [vp, vp, i64, i32]
    lib.khr_mesh_halo_plan.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp]
    lib.khr_mesh_halo_answer.argtypes = [vp, vp, i64, vp, vp, i64]
    lib.khr_mesh_halo_adopt.argtypes = [vp, vp, vp, vp, vp]
    lib.khr_download_updated.argtypes = [vp] + [vp] * 7 + [i64]
    lib.khr_download_updated.restype = i64
    lib.khr_snapshot_updated.argtypes = [vp, C.c_uint32, i64, C.POINTER(vp)]
    lib.khr_take_snapshot.argtypes = [vp, C.POINTER(vp)]
    lib.khr_snapshot_num_blocks.argtypes = [vp]
    lib.khr_snapshot_num_blocks.restype = i64
    lib.khr_snapshot_download.argtypes = [vp] + [vp] * 7 + [i64]
    lib.khr_snapshot_download.restype = i64
    lib.khr_snapshot_download_begin.argtypes = [vp] + [vp] * 7 + [i64]
    lib.khr_snapshot_download_end.argtypes = [vp]
    lib.khr_snapshot_download_end.restype = i64
    lib.khr_snapshot_download_extra.argtypes = [vp, vp, vp, vp, i64]
    lib.khr_snapshot_download_extra.restype = i64
    lib.khr_snapshot_release.argtypes = [vp]
    lib.khr_snapshot_release.restype = None
    lib.khr_mesh_num_vertices.argtypes = [vp]
    lib.khr_mesh_num_vertices.restype = i64
    lib.khr_download_mesh.argtypes = [vp, vp, vp, vp, vp, vp, i64]
    lib.khr_download_mesh.restype = i64
    lib.khr_fetch_mesh.argtypes = [vp, vp]
    lib.khr_fetch_mesh.restype = i64
    lib.khr_fetch_mesh_into.argtypes = [vp, vp, vp, vp, vp, vp]
    lib.khr_weld_mesh.argtypes = [vp, C.c_float, C.POINTER(KhrWeldStats)]
    lib.khr_weld_mesh_into.argtypes = [vp, i32] + [vp] * 7
    lib.khr_merge_map.argtypes = [vp, vp, C.POINTER(KhrMergeRequest), C.POINTER(KhrMergeStats)]
    lib.khr_diff_map.argtypes = [vp, vp, C.POINTER(KhrDiffRequest), C.POINTER(KhrDiffStats)]
    lib.khr_diff_map_into.argtypes = [vp, i32] + [vp] * 11
    lib.khr_segment_map.argtypes = [vp, C.POINTER(KhrSegmentRequest), C.POINTER(KhrSegmentStats)]
    lib.khr_segment_map_into.argtypes = [vp, i32] + [vp] * 10
    lib.khr_voronoi_field.argtypes = [vp, C.POINTER(KhrVoronoiRequest), C.POINTER(KhrVoronoiStats)]
    lib.khr_voronoi_field_into.argtypes = [vp, i32] + [vp] * 9
    lib.khr_places_graph.argtypes = [vp, C.POINTER(KhrPlacesRequest), C.POINTER(KhrPlacesStats)]
    lib.khr_places_graph_from.argtypes = [vp, C.POINTER(KhrPlacesRequest), vp, vp, i32, vp, vp, vp, vp, C.POINTER(KhrPlacesStats)]
    lib.khr_places_graph_into.argtypes = [vp, i32] + [vp] * 14
    lib.khr_places_graph_box.argtypes = [vp, vp, vp]
    lib.khr_travel_field.argtypes = [vp, C.POINTER(KhrTravelRequest), vp, C.c_uint64, i32, C.POINTER(KhrTravelStats)]
    lib.khr_travel_field_from.argtypes = [vp, C.POINTER(KhrTravelRequest), vp, vp, i32, vp, vp, vp, C.c_uint64, C.POINTER(KhrTravelStats)]
    lib.khr_travel_field_box.argtypes = [vp, vp, vp]
    lib.khr_travel_field_into.argtypes = [vp, i32, vp, vp, vp]
    lib.khr_travel_paths.argtypes = [vp, C.c_uint64, vp, i32, C.POINTER(C.c_uint64)]
    lib.khr_travel_paths_into.argtypes = [vp, i32, vp, vp, vp, vp]
    lib.khr_debug_read.argtypes = [vp, vp, i64]
    lib.khr_debug_live_resources.argtypes = [C.POINTER(i64)]
    lib.khr_tick_ingest.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.khr_tick_seed_counts.argtypes = [vp, vp, i32]
    lib.khr_tick_live_bound.argtypes = [vp, vp, i32, i32]
    lib.khr_converted_bytes.argtypes = [vp, i32]
    lib.khr_converted_bytes.restype = C.c_size_t
    lib.khr_export_converted.argtypes = [vp, i32, vp, i32]
    lib.khr_converted_views.argtypes = [vp, vp, i32, vp]
    lib.khr_tick_adopt.argtypes = [vp, vp, vp, i32, i32, vp, vp, vp]
    lib.khr_copy_frame_image.argtypes = [vp, i32, i32, vp]
    lib.khr_tick_integrate.argtypes = [vp, vp, i32, i32, i32, i32]
    lib.khr_last_removed.argtypes = [vp, vp, i64, C.POINTER(i64)]
    lib.khr_process_frame.argtypes = [vp, C.POINTER(KhrSensor), C.POINTER(KhrFrame), i32, C.c_uint32, C.POINTER(i32)]
    lib.khr_ingest_ahead.argtypes = [vp, C.POINTER(KhrSensor), C.POINTER(KhrFrame)]
    lib.khr_ingest_ahead_host.argtypes = [vp, C.POINTER(KhrSensor), C.POINTER(KhrFrame)]
    lib.khr_ingest_cancel.argtypes = [vp]
    lib.khr_ingest_ahead.restype = i32
    lib.khr_reserve_mesh_staging.argtypes = [vp, u64]
    lib.khr_reserve_snapshots.argtypes = [vp, C.c_uint32, i64, i32]
    lib.khr_timing_enable.argtypes = [vp, i32]
    lib.khr_timing_reset.argtypes = [vp]
    lib.khr_timing_get.argtypes = [vp, i32, C.POINTER(C.c_double), C.POINTER(u64)]
    _lib = lib
    return lib


def default_config(**overrides):
    cfg = KhrConfig()
    load_library().khr_default_config(C.byref(cfg))
    for k, v in overrides.items():
        if k == "exact_arithmetic":  # (the C field is the negation: a zero-initialised khr_config means bit-exact values)
            k, v = "relaxed_arithmetic", 0 if v else 1
        if not hasattr(cfg, k):
            raise KeyError(k)
        setattr(cfg, k, v)
    return cfg


def live_resources():
    """Process-wide counts of the HIP resources the library holds right now: (device buffers, page-locked blocks, events, streams)."""
    out = (C.c_int64 * 4)()
    rc = load_library().khr_debug_live_resources(out)
    if rc != 0:
        raise KhronosAmdError("khr_debug_live_resources failed (%d)" % rc)
    return tuple(out)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def slice_voxel_z(height, voxel_size, voxels_per_side):
    """getVoxelKey((0, 0, height)).z as a global voxel index (ASSUMPTIONS.md A.10): block floor, then voxel floor inside the
    block, in float32; a voxel index of -1 / vps that rounding produces stays as it is and names the edge voxel of the
    neighbouring layer.  Same rule as khr_slice_voxel_z (C) and hydra::sliceVoxelZ (C++); needs no library."""
    f32 = np.float32
    h, vs = f32(height), f32(voxel_size)
    if not (np.isfinite(h) and vs > 0 and voxels_per_side >= 1):
        raise ValueError("bad slice arguments (%r, %r, %r)" % (height, voxel_size, voxels_per_side))
    bs = vs * f32(voxels_per_side)
    bz = int(np.floor(h * (f32(1) / bs)))
    v = int(np.floor((h - f32(bz) * bs) * (f32(1) / vs)))
    return bz * int(voxels_per_side) + v


def _byte_view(buf, writable=False):
    """a flat uint8 numpy view of a bytes-like object or array (no copy where the object allows it)"""
    if isinstance(buf, np.ndarray):
        a = buf.reshape(-1).view(np.uint8) if buf.flags.c_contiguous else np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    else:
        a = np.frombuffer(buf, np.uint8)
    if writable and not a.flags.writeable:
        raise ValueError("the buffer is read-only")
    return a


def checkpoint_inspect(buf):
    """khr_checkpoint_inspect: parse and validate the header of a map checkpoint; needs no context and no device.  Returns
    (return code, header dict or None); the error text is khr_last_error's."""
    a = _byte_view(buf)
    h = KhrCheckpointHeader()
    lib = load_library()
    rc = lib.khr_checkpoint_inspect(C.c_void_p(a.ctypes.data if a.size else None), a.size, C.byref(h))
    if rc != 0:
        return rc, None
    out = {n: getattr(h, n) for n, _ in KhrCheckpointHeader._fields_ if n != "offset"}
    out["offset"] = {n: int(h.offset[i]) for i, n in enumerate(CKPT_SECTIONS)}
    return rc, out


class FusionContext:
    """Thin object wrapper over a khr_ctx (one per GPU / per map)."""

    TIMERS = {"tsdf": 0, "tracking": 1, "ever_free": 2, "alloc": 3, "motion_pixels": 4, "mesh": 5, "parse": 6, "band": 7,
              # single kernels (start / stop stamps of the dispatch packet itself)
              "k_mc_count": 8, "k_mc_emit": 9, "k_tracking_update": 10, "k_ever_free": 11, "k_snapshot_pack": 12}

    def __init__(self, cfg):
        self.lib = load_library()
        self.cfg = cfg
        h = C.c_void_p()
        rc = self.lib.khr_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise KhronosAmdError("khr_create failed (%d): %s" % (rc, self.lib.khr_last_error().decode()))
        self.h = h
        self.nvox = cfg.voxels_per_side ** 3

    def close(self):
        # objects that hold frame slots of this context (host_capi.ObjectPipeline) go first
        for d in list(getattr(self, "_dependents", [])):
            d.close()
        self._dependents = []
        if getattr(self, "h", None):
            self.lib.khr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise KhronosAmdError("khr call failed (%d): %s" % (rc, self.lib.khr_last_error().decode()))
        return rc

    def set_stream(self, stream_ptr):
        self._chk(self.lib.khr_set_stream(self.h, C.c_void_p(stream_ptr)))

    def sync(self):
        self._chk(self.lib.khr_sync(self.h))

    @staticmethod
    def make_sensor(width, height, fx, fy, cx, cy, min_range=0.1, max_range=5.0):
        return KhrSensor(width, height, fx, fy, cx, cy, min_range, max_range)

    def upload_frame(self, sensor, stamp_ns, world_T_sensor, depth, color=None, label=None):
        """numpy host buffers.  Returns the frame slot."""
        f = KhrFrame()
        f.timestamp_ns = int(stamp_ns)
        T = np.ascontiguousarray(world_T_sensor, dtype=np.float64).reshape(16)
        for i in range(16):
            f.world_T_sensor[i] = T[i]
        depth = np.ascontiguousarray(depth, dtype=np.float32)
        keep = [depth]
        f.depth = depth.ctypes.data
        if color is not None:
            color = np.ascontiguousarray(color, dtype=np.uint8)
            keep.append(color)
            f.color = color.ctypes.data
        if label is not None:
            label = np.ascontiguousarray(label, dtype=np.int32)
            keep.append(label)
            f.label = label.ctypes.data
        return self._chk(self.lib.khr_upload_frame(self.h, C.byref(sensor), C.byref(f), 0))

    def upload_frame_device(self, sensor, stamp_ns, world_T_sensor, depth_ptr, color_ptr=0, label_ptr=0):
        """HBM-resident buffers given as integer device pointers (e.g. torch tensor .data_ptr())."""
        f = KhrFrame()
        f.timestamp_ns = int(stamp_ns)
        T = np.ascontiguousarray(world_T_sensor, dtype=np.float64).reshape(16)
        for i in range(16):
            f.world_T_sensor[i] = T[i]
        f.depth = depth_ptr
        f.color = color_ptr or None
        f.label = label_ptr or None
        return self._chk(self.lib.khr_upload_frame(self.h, C.byref(sensor), C.byref(f), 1))

    def tick_ingest(self, sensor, frames, count_seeds=True, want_counts=True, counts_device_ptr=0):
        """khr_tick_ingest: `frames` = list of KhrFrame with DEVICE pointers (make_frame).  Returns (slots, seed counts or
        None); want_counts=False does not wait (tick_seed_counts collects later); counts_device_ptr: device int64[n]."""
        n = len(frames)
        arr = (KhrFrame * n)(*frames)
        slots = (C.c_int * n)()
        counts = (C.c_uint32 * n)() if want_counts else None
        self._chk(self.lib.khr_tick_ingest(self.h, C.byref(sensor), arr, n, 1 if count_seeds else 0, slots, counts,
                                           C.c_void_p(counts_device_ptr or None)))
        return list(slots), (list(counts) if want_counts else None)

    def copy_frame_image(self, slot, which, device_ptr):
        """dynamic (0) / object (1) image of a frame slot into a device buffer (int32, W*H), asynchronously."""
        self._chk(self.lib.khr_copy_frame_image(self.h, int(slot), int(which), C.c_void_p(device_ptr)))

    # ---- sender-side ingest: converted planes travel instead of raw frames ----
    def converted_bytes(self, sensor, with_depth=False):
        return int(self.lib.khr_converted_bytes(C.byref(sensor), int(with_depth)))

    def export_converted(self, slot, packed_device_ptr, with_depth=False):
        self._chk(self.lib.khr_export_converted(self.h, int(slot), C.c_void_p(packed_device_ptr), int(with_depth)))

    def converted_frame(self, sensor, packed_device_ptr, stamp_ns, world_T_sensor, with_depth=False, has_color=True, has_label=True):
        """khr_converted_frame whose planes point into one packed buffer (khr_converted_views)"""
        f = KhrConvertedFrame()
        self._chk(self.lib.khr_converted_views(C.byref(sensor), C.c_void_p(packed_device_ptr), int(with_depth), C.byref(f)))
        f.timestamp_ns = int(stamp_ns)
        T = np.ascontiguousarray(world_T_sensor, dtype=np.float64).reshape(16)
        for i in range(16):
            f.world_T_sensor[i] = T[i]
        if not has_color:
            f.rgba = None
        if not has_label:
            f.label = None
        return f

    def tick_adopt(self, sensor, conv_frames, count_seeds=True, want_counts=True, counts_device_ptr=0):
        """khr_tick_adopt: khr_tick_ingest for frames whose converted planes already lie in device memory"""
        n = len(conv_frames)
        arr = (KhrConvertedFrame * n)(*conv_frames)
        slots = (C.c_int * n)()
        counts = (C.c_uint32 * n)() if want_counts else None
        self._chk(self.lib.khr_tick_adopt(self.h, C.byref(sensor), arr, n, 1 if count_seeds else 0, slots, counts,
                                          C.c_void_p(counts_device_ptr or None)))
        return list(slots), (list(counts) if want_counts else None)

    def tick_seed_counts(self, n):
        counts = (C.c_uint32 * n)()
        self._chk(self.lib.khr_tick_seed_counts(self.h, counts, n))
        return list(counts)

    def tick_integrate(self, slots, use_mask=False, object_id=-1, phases=3):
        n = len(slots)
        arr = (C.c_int * n)(*[int(x) for x in slots])
        self._chk(self.lib.khr_tick_integrate(self.h, arr, n, 1 if use_mask else 0, int(object_id), int(phases)))

    PF_OBJECTS = 8
    PF_SNAPSHOT = 32     # with PF_OUTPUT: snapshot of the updated blocks between meshing and archival (take_snapshot)
    PF_INPUT_READY = 16  # device inputs are complete at call time: the ingest may run ahead on the second stream
    PF_INGESTED = 64     # the frame was handed over earlier with ingest_ahead
    PF_INPUT_PINNED = 128  # on_device = False frames in page-locked host memory: copies on the context's own stream, no host wait
    PF_MOTION, PF_TRACKING, PF_OUTPUT = 1, 2, 4

    def make_frame(self, stamp_ns, world_T_sensor, depth_ptr, color_ptr=0, label_ptr=0):
        """pre-built khr_frame for device-resident buffers (reusable across process_frame calls)."""
        f = KhrFrame()
        f.timestamp_ns = int(stamp_ns)
        T = np.ascontiguousarray(world_T_sensor, dtype=np.float64).reshape(16)
        for i in range(16):
            f.world_T_sensor[i] = T[i]
        f.depth = depth_ptr
        f.color = color_ptr or None
        f.label = label_ptr or None
        return f

    def process_frame(self, sensor, frame, on_device=True, flags=3):
        nc = C.c_int(0)
        slot = self._chk(self.lib.khr_process_frame(self.h, C.byref(sensor), C.byref(frame), int(on_device), flags,
                                                    C.byref(nc)))
        return slot, nc.value

    def ingest_ahead(self, sensor, frame):
        """hand the NEXT frame over (khr_ingest_ahead); returns the slot, or None when the look-ahead is not possible now"""
        rc = self.lib.khr_ingest_ahead(self.h, C.byref(sensor), C.byref(frame))
        if rc == -4:  # KHR_ENOTFOUND
            return None
        return self._chk(rc)

    def ingest_ahead_host(self, sensor, frame):
        """khr_ingest_ahead_host: the NEXT frame, in page-locked host memory; None when the look-ahead is not possible now"""
        rc = self.lib.khr_ingest_ahead_host(self.h, C.byref(sensor), C.byref(frame))
        if rc == -4:  # KHR_ENOTFOUND
            return None
        return self._chk(rc)

    def ingest_cancel(self):
        return self.lib.khr_ingest_cancel(self.h) == 0

    def last_removed(self):
        n = C.c_int64(0)
        cap = int(self.cfg.max_blocks)
        out = np.zeros((cap, 3), np.int32)
        self._chk(self.lib.khr_last_removed(self.h, _ptr(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def set_frame_image(self, slot, which, image, device_ptr=None):
        if device_ptr is not None:  # device buffer (int32, W*H)
            self._chk(self.lib.khr_set_frame_image(self.h, slot, which, C.c_void_p(device_ptr), 1))
        elif image is None:
            self._chk(self.lib.khr_set_frame_image(self.h, slot, which, None, 0))
        else:
            image = np.ascontiguousarray(image, dtype=np.int32)
            self._chk(self.lib.khr_set_frame_image(self.h, slot, which, _ptr(image), 0))

    def download_frame(self, slot, shape, range_image=True, vertex_map=False, dynamic_image=False, object_image=False):
        h, w = shape
        r = np.empty((h, w), np.float32) if range_image else None
        v = np.empty((h, w, 3), np.float32) if vertex_map else None
        d = np.empty((h, w), np.int32) if dynamic_image else None
        self._chk(self.lib.khr_download_frame(self.h, slot, _ptr(r), _ptr(v), _ptr(d)))
        if not object_image:
            return r, v, d
        o = np.empty((h, w), np.int32)
        self._chk(self.lib.khr_download_frame_image(self.h, slot, 1, _ptr(o)))
        return r, v, d, o

    def integrate(self, slot, allocate_blocks=True, use_mask=False, object_id=-1):
        self._chk(self.lib.khr_integrate(self.h, slot, int(allocate_blocks), int(use_mask), int(object_id)))

    def integrate_shared(self, src, slot, allocate_blocks=False, use_mask=False, object_id=-1):
        """khr_integrate_shared: integrate frame `slot` of context `src` into THIS map (the object extractor's mini-map)."""
        self._chk(self.lib.khr_integrate_shared(self.h, src.h, int(slot), int(allocate_blocks), int(use_mask), int(object_id)))

    def integrate_shared_batch(self, src, slots, object_ids=None, allocate_blocks=False, use_mask=False):
        """khr_integrate_shared_batch: the frames `slots` of context `src`, in order, in one call (one launch for 8^3 maps)."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ids = None if object_ids is None else np.ascontiguousarray(object_ids, dtype=np.int32)
        self._chk(self.lib.khr_integrate_shared_batch(self.h, src.h, _ptr(sl), None if ids is None else _ptr(ids), len(sl),
                                                      int(allocate_blocks), int(use_mask)))

    def update_tracking(self, stamp_ns):
        self._chk(self.lib.khr_update_tracking(self.h, int(stamp_ns)))

    def update_tracking_phase(self, stamp_ns, phase):
        self._chk(self.lib.khr_update_tracking_phase(self.h, int(stamp_ns), int(phase)))

    HALO_WORDS = 66

    def export_halo(self, cap_records, device_ptr=None):
        """host numpy [cap, 66] uint64, or write into an HBM buffer given as an integer pointer."""
        if device_ptr is not None:
            self._chk(self.lib.khr_export_halo(self.h, C.c_void_p(device_ptr), int(cap_records), 1))
            return None
        out = np.zeros((cap_records, self.HALO_WORDS), np.uint64)
        self._chk(self.lib.khr_export_halo(self.h, _ptr(out), int(cap_records), 0))
        return out

    def import_halo(self, records=None, n_records=0, device_ptr=None):
        if device_ptr is not None:
            self._chk(self.lib.khr_import_halo(self.h, C.c_void_p(device_ptr), int(n_records), 1))
            return
        if records is None or len(records) == 0:
            self._chk(self.lib.khr_import_halo(self.h, None, 0, 0))
            return
        records = np.ascontiguousarray(records, dtype=np.uint64).reshape(-1, self.HALO_WORDS)
        self._chk(self.lib.khr_import_halo(self.h, _ptr(records), records.shape[0], 0))

    def detect_motion(self, slot):
        return self._chk(self.lib.khr_detect_motion(self.h, slot))

    def motion_keys(self, slot, shape=None, device_ptr=None):
        """per-pixel voxel keys of this rank's shard (0 = not mine / skipped); returns (keys or None, n_seed_pixels)."""
        ns = C.c_uint32(0)
        if device_ptr is not None:
            self._chk(self.lib.khr_motion_keys(self.h, slot, C.c_void_p(device_ptr), 1, C.byref(ns)))
            return None, ns.value
        out = np.zeros(shape, np.uint64)
        self._chk(self.lib.khr_motion_keys(self.h, slot, _ptr(out), 0, C.byref(ns)))
        return out, ns.value

    def detect_motion_from_keys(self, slot, keys=None, device_ptr=None):
        if device_ptr is not None:
            return self._chk(self.lib.khr_detect_motion_from_keys(self.h, slot, C.c_void_p(device_ptr), 1))
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        return self._chk(self.lib.khr_detect_motion_from_keys(self.h, slot, _ptr(keys), 0))

    def dynamic_clusters(self, slot):
        n = self._chk(self.lib.khr_get_dynamic_clusters(self.h, slot, None, 0))
        arr = (KhrCluster * max(n, 1))()
        n = self._chk(self.lib.khr_get_dynamic_clusters(self.h, slot, arr, n))
        return [dict(id=a.id, num_pixels_listed=a.num_pixels_listed, num_pixels_painted=a.num_pixels_painted,
                     bbox_min=np.array(a.bbox_min[:]), bbox_max=np.array(a.bbox_max[:]), centroid=np.array(a.centroid[:]))
                for a in arr[:n]]

    # -- object detection / track measurements (ConnectedSemantics, MaxIoUTracker voxel sets) --
    def configure_object_detector(self, object_labels, use_3d=True, grid_size=0.1, max_range=0.0, min_cluster_size=0,
                                  max_cluster_size=-1, use_full_connectivity=True):
        labels = np.ascontiguousarray(object_labels, dtype=np.int32)
        oc = KhrObjectDetectorConfig(int(use_full_connectivity), int(min_cluster_size), int(max_cluster_size), int(use_3d),
                                     float(grid_size), float(max_range), labels.ctypes.data_as(C.POINTER(C.c_int32)), labels.size)
        self._chk(self.lib.khr_configure_object_detector(self.h, C.byref(oc)))

    def detect_objects(self, slot):
        return self._chk(self.lib.khr_detect_objects(self.h, slot))

    def semantic_clusters(self, slot):
        n = self._chk(self.lib.khr_get_semantic_clusters(self.h, slot, None, 0))
        arr = (KhrCluster * max(n, 1))()
        n = self._chk(self.lib.khr_get_semantic_clusters(self.h, slot, arr, n))
        return [dict(id=a.id, semantic_id=a.semantic_id, num_pixels=a.num_pixels_listed, bbox_min=np.array(a.bbox_min[:]),
                     bbox_max=np.array(a.bbox_max[:]), centroid=np.array(a.centroid[:])) for a in arr[:n]]

    def pixel_iou(self, slot, refs, max_id):
        """MaxIoUTracker track_by = pixels: refs = [(slot, which, id), ...] (<= 32) -> (n_points[r], inter[r, max_id + 1])."""
        r = np.ascontiguousarray(np.array(refs, np.int32).reshape(-1, 3))
        n_points = np.zeros(max(len(r), 1), np.uint32)
        inter = np.zeros((max(len(r), 1), max_id + 1), np.uint32)
        self._chk(self.lib.khr_pixel_iou(self.h, slot, _ptr(r), len(r), int(max_id), _ptr(n_points), _ptr(inter)))
        return n_points[:len(r)], inter[:len(r)]

    def forward_instances(self, slot, max_range=0.0, background_ids=(), max_id=255):
        """InstanceForwarding::extractSemanticClusters: per-id summaries of the label image (ids present only)."""
        bg = np.ascontiguousarray(sorted(background_ids), dtype=np.int32)
        arr = (KhrCluster * (max_id + 1))()
        n = self._chk(self.lib.khr_forward_instances(self.h, slot, float(max_range), _ptr(bg) if bg.size else None, int(bg.size),
                                                     int(max_id), arr))
        out = [dict(id=a.id, num_pixels=a.num_pixels_listed, bbox_min=np.array(a.bbox_min[:]), bbox_max=np.array(a.bbox_max[:]),
                    centroid=np.array(a.centroid[:])) for a in arr if a.num_pixels_listed]
        assert len(out) == n
        return out

    def cluster_voxels(self, slot, which, voxel_size):
        """distinct (cluster id, voxel) pairs of the dynamic (which=0) / object (which=1) image: (ids[n], voxels[n,3])."""
        n = self.lib.khr_cluster_voxels(self.h, slot, which, float(voxel_size), None, None, 0)
        self._chk(n)
        ids = np.zeros(max(n, 1), np.int32)
        vox = np.zeros((max(n, 1), 3), np.int64)
        n2 = self.lib.khr_cluster_voxels(self.h, slot, which, float(voxel_size), _ptr(ids), _ptr(vox), n)
        self._chk(n2)
        return ids[:n], vox[:n]

    def configure_object_voxel_sets(self, voxel_size):
        """the tracker's voxel size: the detector's id remap then also collects the object image's voxel sets (0 = off)."""
        self._chk(self.lib.khr_configure_object_voxel_sets(self.h, float(voxel_size)))

    def cluster_voxels_launch(self, slot, which, voxel_size):
        self._chk(self.lib.khr_cluster_voxels_launch(self.h, slot, which, float(voxel_size)))

    def cluster_voxels_fetch(self, which):
        n = self.lib.khr_cluster_voxels_fetch(self.h, which, None, None, 0)
        self._chk(n)
        ids = np.zeros(max(n, 1), np.int32)
        vox = np.zeros((max(n, 1), 3), np.int64)
        self._chk(self.lib.khr_cluster_voxels_fetch(self.h, which, _ptr(ids), _ptr(vox), n))
        return ids[:n], vox[:n]

    def generate_mesh(self, only_mesh_updated=True, clear_flag=True):
        self._chk(self.lib.khr_generate_mesh(self.h, int(only_mesh_updated), int(clear_flag)))

    def reset_inactive(self):
        n = C.c_int64(0)
        cap = int(self.cfg.max_blocks)
        out = np.zeros((cap, 3), np.int32)
        self._chk(self.lib.khr_reset_inactive(self.h, _ptr(out), cap, C.byref(n)))
        return out[: n.value].copy()

    def reset_inactive_async(self):
        """no host round trip; the archived indices stay on the device (fetch with last_removed())."""
        self._chk(self.lib.khr_reset_inactive(self.h, None, 0, None))

    def mark_all_inactive(self):
        self._chk(self.lib.khr_mark_all_inactive(self.h))

    def reset_map(self, voxel_size, truncation_distance):
        """empty map at a new resolution, allocations kept (object mini-maps are reused between objects)"""
        self._chk(self.lib.khr_reset_map(self.h, float(voxel_size), float(truncation_distance)))
        self.cfg.voxel_size, self.cfg.truncation_distance = float(voxel_size), float(truncation_distance)

    def clear_updated(self):
        self._chk(self.lib.khr_clear_updated(self.h))

    def allocate_blocks(self, indices):
        idx = np.ascontiguousarray(indices, dtype=np.int32).reshape(-1, 3)
        self._chk(self.lib.khr_allocate_blocks(self.h, _ptr(idx), idx.shape[0]))

    def begin_object_map(self, voxel_size, truncation_distance, lo, hi):
        """khr_begin_object_map: reset_map + allocate_blocks of the dense block box lo <= index <= hi, in two launches."""
        lo3 = np.ascontiguousarray(lo, dtype=np.int32).reshape(3)
        hi3 = np.ascontiguousarray(hi, dtype=np.int32).reshape(3)
        self._chk(self.lib.khr_begin_object_map(self.h, float(voxel_size), float(truncation_distance), _ptr(lo3), _ptr(hi3)))
        self.cfg.voxel_size, self.cfg.truncation_distance = float(voxel_size), float(truncation_distance)

    def integrate_prune_batch(self, src, slots, object_ids, min_confidence, min_observations, use_mask=False):
        """khr_integrate_prune_batch: integrate_shared_batch(allocate_blocks=False) + object_prune; returns the pruned count."""
        sl = np.ascontiguousarray(slots, dtype=np.int32)
        ids = None if object_ids is None else np.ascontiguousarray(object_ids, dtype=np.int32)
        n = C.c_int64(0)
        self._chk(self.lib.khr_integrate_prune_batch(self.h, src.h, _ptr(sl), None if ids is None else _ptr(ids), len(sl),
                                                     int(use_mask), min_confidence, min_observations, C.byref(n)))
        return n.value

    def object_prune(self, min_confidence, min_observations):
        n = C.c_int64(0)
        self._chk(self.lib.khr_object_prune(self.h, min_confidence, min_observations, C.byref(n)))
        return n.value

    def stats(self):
        s = KhrStats()
        self._chk(self.lib.khr_get_stats(self.h, C.byref(s)))
        return {n: (list(getattr(s, n)) if n == "seed_wait_hist" else getattr(s, n)) for n, _ in KhrStats._fields_}

    DIGEST_LAYERS = ("distance", "weight", "color", "last_observed", "last_occupied", "flags", "sem_label", "likelihoods",
                     "block_flags", "index", "n_blocks", "reserved")

    def map_digest(self):
        """khr_map_digest: order-independent 64-bit digests of the whole map, one per layer (np.uint64[12], DIGEST_LAYERS)."""
        out = np.zeros(12, np.uint64)
        self._chk(self.lib.khr_map_digest(self.h, _ptr(out)))
        return out

    def num_blocks(self):
        return self._chk(self.lib.khr_num_blocks(self.h))

    def block_indices(self, only_updated=False):
        n = self._chk(self.lib.khr_block_indices(self.h, None, 0, int(only_updated)))
        out = np.zeros((max(n, 1), 3), np.int32)
        n = self._chk(self.lib.khr_block_indices(self.h, _ptr(out), n, int(only_updated)))
        return out[:n]

    def download_block(self, idx, likelihoods=True):
        nv, K = self.nvox, max(1, self.cfg.num_labels)
        b = {
            "distance": np.empty(nv, np.float32), "weight": np.empty(nv, np.float32),
            "color": np.empty((nv, 4), np.uint8), "last_observed": np.empty(nv, np.uint64),
            "last_occupied": np.empty(nv, np.uint64), "flags": np.empty(nv, np.uint8),
            "sem_label": np.empty(nv, np.uint32),
            "likelihoods": np.zeros((K, nv), np.float32) if (likelihoods and self.cfg.with_semantics) else None,
        }
        bf = np.zeros(1, np.uint8)
        self._chk(self.lib.khr_download_block(
            self.h, int(idx[0]), int(idx[1]), int(idx[2]), _ptr(b["distance"]), _ptr(b["weight"]), _ptr(b["color"]),
            _ptr(b["last_observed"]), _ptr(b["last_occupied"]), _ptr(b["flags"]), _ptr(b["sem_label"]),
            _ptr(b["likelihoods"]), _ptr(bf)))
        b["block_flags"] = int(bf[0])
        return b

    # ---- map checkpoints (khr_checkpoint_*; the format: include/khronos_amd.h, numpy codec: khronos_amd/checkpoint.py) ----
    def checkpoint_size(self):
        """(bytes, blocks) of a checkpoint of the live map"""
        nb, nk = C.c_uint64(0), C.c_int64(0)
        self._chk(self.lib.khr_checkpoint_size(self.h, C.byref(nb), C.byref(nk)))
        return nb.value, nk.value

    def save_map_into(self, out):
        """khr_checkpoint_save into a writable buffer; returns (return code, stream length) without raising"""
        a = _byte_view(out, writable=True)
        n = C.c_uint64(0)
        rc = self.lib.khr_checkpoint_save(self.h, C.c_void_p(a.ctypes.data if a.size else None), a.size, C.byref(n))
        return rc, n.value

    def save_map(self, out=None):
        """The live map as one checkpoint stream: `bytes`, or -- with `out`, a writable buffer -- the number of bytes written."""
        if out is not None:
            rc, n = self.save_map_into(out)
            self._chk(rc)
            return n
        nbytes, _ = self.checkpoint_size()
        buf = np.empty(nbytes, np.uint8)
        rc, n = self.save_map_into(buf)
        self._chk(rc)
        return buf[:n].tobytes()

    def load_map_rc(self, buf, ptr=None, nbytes=0):
        """khr_checkpoint_load; returns (return code, kept blocks) without raising.  ptr / nbytes: a raw host pointer instead"""
        kept = C.c_int64(0)
        if ptr is not None:
            return self.lib.khr_checkpoint_load(self.h, C.c_void_p(ptr), int(nbytes), C.byref(kept)), kept.value
        a = _byte_view(buf)
        rc = self.lib.khr_checkpoint_load(self.h, C.c_void_p(a.ctypes.data if a.size else None), a.size, C.byref(kept))
        return rc, kept.value

    def load_map(self, buf):
        """Restore a checkpoint stream into this context's EMPTY map; returns the number of blocks kept (a sharded context keeps
        the blocks it owns)."""
        rc, kept = self.load_map_rc(buf)
        self._chk(rc)
        return kept

    SLICE_FIELDS = ("block_xy", "positions", "distance", "weight", "last_observed", "flags")

    def map_slice_into(self, voxel_z, cap, out):
        """khr_map_slice into caller arrays (`out`: SLICE_FIELDS -> contiguous array or None); returns (return code, voxel count)
        without raising, so that callers can see KHR_ENOMEM and the true count."""
        n = C.c_int64(0)
        rc = self.lib.khr_map_slice(self.h, int(voxel_z), int(cap), *[_ptr(out.get(k)) for k in self.SLICE_FIELDS], C.byref(n))
        return rc, n.value

    def map_slice(self, voxel_z):
        """One z-plane of the live map (khr_map_slice): dict with voxel_z, block_xy (blocks, 2) int32 sorted by (bx, by),
        positions (n, 3) float32 voxel centres, distance, weight, last_observed (uint64), flags (uint8); voxels of a block
        x-outer / y-inner."""
        vps = self.cfg.voxels_per_side
        cap = getattr(self, "_slice_hint", 0)
        while True:
            out = {"block_xy": np.zeros((cap // (vps * vps), 2), np.int32), "positions": np.zeros((cap, 3), np.float32),
                   "distance": np.zeros(cap, np.float32), "weight": np.zeros(cap, np.float32),
                   "last_observed": np.zeros(cap, np.uint64), "flags": np.zeros(cap, np.uint8)}
            rc, n = self.map_slice_into(voxel_z, cap, out)
            if rc == KHR_ENOMEM and n > cap:
                cap = n
                continue
            self._chk(rc)
            break
        self._slice_hint = n
        res = {k: v[: n // (vps * vps)] if k == "block_xy" else v[:n] for k, v in out.items()}
        res["voxel_z"] = int(voxel_z)
        return res

    RENDER_FIELDS = (("depth", np.float32, ()), ("normal", np.float32, (3,)), ("color", np.uint8, (4,)), ("label", np.uint32, ()),
                     ("flags", np.uint8, ()), ("status", np.uint8, ()))

    @staticmethod
    def render_request(sensor, world_T_sensor, step_voxels=0.0, min_weight=0.0):
        rq = KhrRenderRequest()
        rq.sensor = sensor
        T = np.ascontiguousarray(world_T_sensor, dtype=np.float64).reshape(16)
        for i in range(16):
            rq.world_T_sensor[i] = T[i]
        rq.step_voxels, rq.min_weight = step_voxels, min_weight
        return rq

    def render_view_into(self, request, out, on_device=False, want_stats=True):
        """khr_render_view into caller buffers (`out`: RENDER_FIELDS name -> contiguous array, or an integer device pointer with
        on_device; absent / None = not rendered).  `request` may be None (the NULL request).  Returns (return code, stats dict or
        None) without raising."""
        st = KhrRenderStats()
        ptrs = []
        for name, _, _ in self.RENDER_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        rc = self.lib.khr_render_view(self.h, None if request is None else C.byref(request), int(on_device), *ptrs,
                                      C.byref(st) if want_stats else None)
        stats = {n: int(getattr(st, n)) for n, _ in KhrRenderStats._fields_} if (want_stats and rc == 0) else None
        return rc, stats

    def render_view(self, sensor, pose, step_voxels=0, min_weight=0, device=False):
        """The live map seen from `pose` through `sensor` (khr_render_view, ASSUMPTIONS.md A.12): dict with depth (H, W) float32,
        normal (H, W, 3) float32 in the world frame, color (H, W, 4) uint8, label (H, W) uint32, flags (H, W) uint8 (VOX_* bits),
        status (H, W) uint8 (0 none, 1 hit, 2 blocked) and stats (n_hit, n_blocked, n_samples_total, n_samples_evaluated).
        device=True: the images are torch tensors on the context's device; the kernel writes every pixel on the context's stream
        and the call returns when the counters have arrived, i.e. after the images are complete."""
        H, W = int(sensor.height), int(sensor.width)
        rq = self.render_request(sensor, pose, step_voxels, min_weight)
        if device:
            import torch
            dev = torch.device("cuda", self.cfg.device)
            tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint32: torch.int32}
            out = {n: torch.empty((max(H, 0), max(W, 0)) + sh, dtype=tdt[dt], device=dev) for n, dt, sh in self.RENDER_FIELDS}
            rc, stats = self.render_view_into(rq, {n: t.data_ptr() for n, t in out.items()}, on_device=True)
        else:
            out = {n: np.zeros((max(H, 0), max(W, 0)) + sh, dt) for n, dt, sh in self.RENDER_FIELDS}
            rc, stats = self.render_view_into(rq, out)
        self._chk(rc)
        out["stats"] = stats
        return out

    QUERY_FIELDS = (("distance", np.float32, ()), ("gradient", np.float32, (3,)), ("weight", np.float32, ()), ("color", np.uint8, (4,)),
                    ("label", np.uint32, ()), ("flags", np.uint8, ()), ("last_observed", np.uint64, ()), ("status", np.uint8, ()))

    def query_points_into(self, n, points, out, min_weight=0.0, on_device=False, want_stats=True):
        """khr_query_points into caller buffers.  `points`: a contiguous float32 array of 3 * n values, or an integer device pointer
        with on_device, or None (the NULL pointer); `out`: QUERY_FIELDS name -> contiguous array, or an integer device pointer with
        on_device; absent / None = not computed.  Returns (return code, stats dict or None) without raising."""
        st = KhrQueryStats()
        ptrs = []
        for name, _, _ in self.QUERY_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        pts = None if points is None else (C.c_void_p(int(points)) if on_device else _ptr(points))
        rc = self.lib.khr_query_points(self.h, int(n), pts, float(min_weight), int(on_device), *ptrs, C.byref(st) if want_stats else None)
        stats = {k: int(getattr(st, k)) for k, _ in KhrQueryStats._fields_} if (want_stats and rc == 0) else None
        return rc, stats

    def query_points(self, points, min_weight=0, device=False):
        """The live map at world points (khr_query_points, ASSUMPTIONS.md A.13).  `points`: (n, 3) float32, metres, world frame (a
        torch tensor on the context's device with device=True).  Returns a dict: distance (n,) float32, gradient (n, 3) float32
        (d(distance) / d(metres), not normalised), and of the voxel each point lies in weight (n,) float32, color (n, 4) uint8,
        label (n,) uint32, flags (n,) uint8 (VOX_* bits), last_observed (n,) uint64; status (n,) uint8 (KHR_QP_* bits) and stats
        (n_value, n_gradient, n_voxel).  Every output of a point whose status bit is clear is zero.  device=True: the outputs are
        torch tensors on the context's device, complete when the call returns (it waits for the counters)."""
        if device:
            import torch
            dev = torch.device("cuda", self.cfg.device)
            pts = torch.as_tensor(points, dtype=torch.float32, device=dev).reshape(-1, 3).contiguous()
            n = int(pts.shape[0])
            tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64}
            out = {k: torch.empty((n,) + sh, dtype=tdt[dt], device=dev) for k, dt, sh in self.QUERY_FIELDS}
            rc, stats = self.query_points_into(n, pts.data_ptr(), {k: t.data_ptr() for k, t in out.items()}, min_weight, on_device=True)
        else:
            pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
            n = len(pts)
            out = {k: np.zeros((n,) + sh, dt) for k, dt, sh in self.QUERY_FIELDS}
            rc, stats = self.query_points_into(n, pts, out, min_weight)
        self._chk(rc)
        out["stats"] = stats
        return out

    DF_FIELDS = (("distance", np.float32), ("d2", np.int32), ("status", np.uint8))

    @staticmethod
    def df_request(origin, dims, ratio=1, max_distance=1.0, min_weight=0.0, surface_distance=0.0, unknown_is_obstacle=False,
                   positive_only=False):
        """a khr_df_request: `origin` (first cell) and `dims` (cells per axis) as x, y, z"""
        rq = KhrDfRequest()
        for a in range(3):
            rq.origin[a], rq.dims[a] = int(origin[a]), int(dims[a])
        rq.ratio = int(ratio)
        rq.min_weight, rq.max_distance, rq.surface_distance = float(min_weight), float(max_distance), float(surface_distance)
        rq.unknown_is_obstacle, rq.positive_only = int(bool(unknown_is_obstacle)), int(bool(positive_only))
        return rq

    def distance_field_into(self, request, out, on_device=False, want_stats=True):
        """khr_distance_field into caller buffers (`out`: DF_FIELDS name -> contiguous array, or an integer device pointer with
        on_device; absent / None = not written).  `request` may be None (the NULL request).  Returns (return code, stats dict or
        None) without raising."""
        st = KhrDfStats()
        ptrs = []
        for name, _ in self.DF_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        rc = self.lib.khr_distance_field(self.h, None if request is None else C.byref(request), int(on_device), *ptrs,
                                         C.byref(st) if want_stats else None)
        stats = {k: int(getattr(st, k)) for k, _ in KhrDfStats._fields_} if (want_stats and rc == 0) else None
        return rc, stats

    def distance_field(self, origin, dims, ratio=1, max_distance=1.0, min_weight=0.0, surface_distance=0.0, unknown_is_obstacle=False,
                       positive_only=False, device=False):
        """The exact Euclidean distance field of a box of the live map (khr_distance_field, ASSUMPTIONS.md A.15).  `origin`: the
        box's first cell, `dims`: cells per axis, both (x, y, z); a cell is `ratio` voxels wide.  Only the cells of the box take
        part: pad the box by max_distance for values that are exact with respect to the whole map.  Returns a dict of arrays
        shaped (nz, ny, nx): distance float32 (metres, negative inside obstacles unless positive_only, +-max_distance out of
        range), d2 int32 (squared cell units, +-KHR_DF_FAR out of range), status uint8 (KHR_DF_* bits); cell_size; and stats
        (n_observed, n_obstacle, n_free, n_in_range).  device=True: the arrays are torch tensors on the context's device, complete
        when the call returns (it waits for the counters)."""
        rq = self.df_request(origin, dims, ratio, max_distance, min_weight, surface_distance, unknown_is_obstacle, positive_only)
        shape = tuple(max(int(d), 0) for d in (dims[2], dims[1], dims[0]))
        if device:
            import torch
            dev = torch.device("cuda", self.cfg.device)
            tdt = {np.float32: torch.float32, np.int32: torch.int32, np.uint8: torch.uint8}
            out = {k: torch.empty(shape, dtype=tdt[dt], device=dev) for k, dt in self.DF_FIELDS}
            rc, stats = self.distance_field_into(rq, {k: t.data_ptr() for k, t in out.items()}, on_device=True)
        else:
            out = {k: np.zeros(shape, dt) for k, dt in self.DF_FIELDS}
            rc, stats = self.distance_field_into(rq, out)
        self._chk(rc)
        out["cell_size"] = float(np.float32(self.cfg.voxel_size) * np.float32(int(ratio)))
        out["stats"] = stats
        return out

    def align_request(self, pose, points=None, depth=None, sensor=None, stride=1, weights=None, min_weight=0.0, gate=0.0, huber_delta=0.0,
                      device=False, n=None):
        """a khr_align_request plus the arrays it points into (keep the second value alive for the duration of the call).  Host
        form: `points` (n, 3) / `depth` (H, W) / `weights` are converted to contiguous float32 arrays; device=True: they are integer
        device pointers (points: pass `n`)."""
        rq = KhrAlignRequest()
        keep = []

        def ptr(a):
            if a is None:
                return None
            if device:
                return int(a)
            a = np.ascontiguousarray(a, dtype=np.float32)
            keep.append(a)
            return a.ctypes.data

        if points is not None:
            if device and n is None:
                raise ValueError("a device point list needs n, the number of points")
            rq.n = int(n) if n is not None else int(np.asarray(points).size // 3)
            rq.points = ptr(points)
        elif n is not None:
            rq.n = int(n)
        if depth is not None:
            rq.depth = ptr(depth)
        if sensor is not None:
            rq.sensor = sensor
        rq.stride = int(stride)
        rq.weights = ptr(weights)
        T = np.ascontiguousarray(pose, dtype=np.float64).reshape(16)
        for i in range(16):
            rq.world_T_source[i] = T[i]
        rq.min_weight, rq.gate, rq.huber_delta = float(min_weight), float(gate), float(huber_delta)
        return rq, keep

    def align_linearize_into(self, request, words, on_device=False):
        """khr_align_linearize into `words` (a uint64 array of at least KHR_ALIGN_WORDS entries, or None for the NULL pointer);
        `request` may be None.  Returns the return code without raising."""
        return self.lib.khr_align_linearize(self.h, None if request is None else C.byref(request), int(on_device), _ptr(words))

    def align_linearize(self, pose, points=None, depth=None, sensor=None, stride=1, weights=None, min_weight=0.0, gate=0.0,
                        huber_delta=0.0, device=False, n=None):
        """One linearisation of the point-to-map registration at `pose` (khr_align_linearize, ASSUMPTIONS.md A.14): the 32 uint64
        words -- H's upper triangle (21), b (6), e, n_inlier, n_gradient, n_source, the sum of w rho -- of a point list (`points` (n, 3), source
        frame) or of a depth image (`depth` (H, W), `sensor`, `stride`).  device=True: points / depth / weights are device
        pointers."""
        rq, keep = self.align_request(pose, points, depth, sensor, stride, weights, min_weight, gate, huber_delta, device, n)
        words = np.zeros(KHR_ALIGN_WORDS, np.uint64)
        self._chk(self.align_linearize_into(rq, words, on_device=device))
        return words

    @staticmethod
    def align_unpack(words):
        """(H (6, 6) float64, b (6,), e, n_inlier) from the words of align_linearize"""
        v = np.asarray(words, np.uint64).view(np.int64).astype(np.float64) * 2.0 ** -24
        H = np.zeros((6, 6))
        k = 0
        for a in range(6):
            for b in range(a, 6):
                H[a, b] = H[b, a] = v[k]
                k += 1
        return H, v[21:27].copy(), float(v[27]), int(words[28])

    def align_frame_into(self, request, pose_out, on_device=False, max_iterations=10, min_inliers=64, lam=1e-4, eps_rot=1e-5, eps_trans=1e-5,
                         default_options=False):
        """khr_align_frame: (return code, result dict) without raising; `pose_out`: float64 array of 16 (or None)."""
        opt = KhrAlignOptions(int(max_iterations), int(min_inliers), float(lam), float(eps_rot), float(eps_trans))
        res = KhrAlignResult()
        rc = self.lib.khr_align_frame(self.h, None if request is None else C.byref(request), int(on_device),
                                      None if default_options else C.byref(opt), _ptr(pose_out), C.byref(res))
        out = dict(iterations=int(res.iterations), converged=bool(res.converged), n_inlier_first=int(res.n_inlier_first),
                   n_inlier_last=int(res.n_inlier_last), rmse_first=float(res.rmse_first), rmse_last=float(res.rmse_last),
                   H=np.array(res.H[:], np.float64), b=np.array(res.b[:], np.float64))
        return rc, out

    def _align(self, rq, device, opts):
        pose = np.zeros(16, np.float64)
        rc, res = self.align_frame_into(rq, pose, on_device=device, **opts)
        if rc != KHR_ENOTFOUND:
            self._chk(rc)
        res["found"] = rc == 0
        return pose.reshape(4, 4), res

    def align_points(self, points, prior, weights=None, min_weight=0.0, gate=0.0, huber_delta=0.0, device=False, n=None, **options):
        """Register a point list (source frame) against the live map, starting from `prior` (4x4 world_T_source): returns (pose
        (4, 4) float64, result dict).  result["found"] is False when the map did not constrain the pose (KHR_ENOTFOUND): the pose
        returned is then the prior.  options: max_iterations, min_inliers, lam, eps_rot, eps_trans."""
        rq, keep = self.align_request(prior, points=points, weights=weights, min_weight=min_weight, gate=gate, huber_delta=huber_delta,
                                      device=device, n=n)
        return self._align(rq, device, options)

    def align_depth(self, depth, sensor, prior, stride=1, weights=None, min_weight=0.0, gate=0.0, huber_delta=0.0, device=False, **options):
        """The same for a depth image seen through `sensor`, every `stride`-th pixel of every `stride`-th row."""
        rq, keep = self.align_request(prior, depth=depth, sensor=sensor, stride=stride, weights=weights, min_weight=min_weight, gate=gate,
                                      huber_delta=huber_delta, device=device)
        return self._align(rq, device, options)

    def mesh_halo_words(self):
        v = self.cfg.voxels_per_side
        return 4 + 3 * 6 * v * v

    def mesh_halo_requests(self, cap, only_mesh_updated=True, device_ptr=None):
        if device_ptr is not None:
            return None, self._chk(self.lib.khr_mesh_halo_requests(self.h, C.c_void_p(device_ptr), cap, int(only_mesh_updated), 1))
        out = np.zeros(cap, np.uint64)
        n = self._chk(self.lib.khr_mesh_halo_requests(self.h, _ptr(out), cap, int(only_mesh_updated), 0))
        return out, n

    def mesh_halo_export(self, requests, cap_records, req_ptr=None, n_req=0, out_ptr=None):
        if out_ptr is not None:
            self._chk(self.lib.khr_mesh_halo_export(self.h, C.c_void_p(req_ptr), n_req, C.c_void_p(out_ptr), cap_records, 1))
            return None
        requests = np.ascontiguousarray(requests, dtype=np.uint64).reshape(-1)
        out = np.zeros((cap_records, self.mesh_halo_words()), np.uint32)
        self._chk(self.lib.khr_mesh_halo_export(self.h, _ptr(requests), requests.size, _ptr(out), cap_records, 0))
        return out

    # compact form (khr_mesh_halo_requests_sorted / _plan / _answer / _adopt): device buffers only
    def mesh_halo_requests_sorted(self, device_ptr, cap, only_mesh_updated=True):
        return self._chk(self.lib.khr_mesh_halo_requests_sorted(self.h, C.c_void_p(device_ptr), cap, int(only_mesh_updated)))

    def mesh_halo_plan(self, headers):
        """headers: u64 [world, 8 * world] (host).  Returns sendcounts, sdispls, recvcounts, rdispls (u32 words, u64 arrays)."""
        w = self.cfg.world_size
        headers = np.ascontiguousarray(headers, dtype=np.uint64).reshape(w, 8 * w)
        out = [np.zeros(w, np.uint64) for _ in range(4)]
        self._chk(self.lib.khr_mesh_halo_plan(w, self.cfg.rank, self.cfg.voxels_per_side, _ptr(headers), *[_ptr(o) for o in out]))
        return out

    def mesh_halo_answer(self, all_requests_ptr, cap, headers, records_ptr, cap_words):
        headers = np.ascontiguousarray(headers, dtype=np.uint64)
        return self._chk(self.lib.khr_mesh_halo_answer(self.h, C.c_void_p(all_requests_ptr), cap, _ptr(headers), C.c_void_p(records_ptr), cap_words))

    def mesh_halo_adopt(self, own_requests_ptr=None, own_header=None, records_ptr=None, rdispls=None):
        if own_requests_ptr is None:
            self._chk(self.lib.khr_mesh_halo_adopt(self.h, None, None, None, None))
            return
        own_header = np.ascontiguousarray(own_header, dtype=np.uint64)
        rdispls = np.ascontiguousarray(rdispls, dtype=np.uint64)
        self._chk(self.lib.khr_mesh_halo_adopt(self.h, C.c_void_p(own_requests_ptr), _ptr(own_header), C.c_void_p(records_ptr), _ptr(rdispls)))

    def mesh_halo_import(self, records=None, device_ptr=None, n_records=0):
        if device_ptr is not None:
            self._chk(self.lib.khr_mesh_halo_import(self.h, C.c_void_p(device_ptr), n_records, 1))
            return
        if records is None or len(records) == 0:
            self._chk(self.lib.khr_mesh_halo_import(self.h, None, 0, 0))
            return
        records = np.ascontiguousarray(records, dtype=np.uint32).reshape(-1, self.mesh_halo_words())
        self._chk(self.lib.khr_mesh_halo_import(self.h, _ptr(records), records.shape[0], 0))

    def download_updated(self):
        """VolumetricMap::cloneUpdated in one packed transfer."""
        n = len(self.block_indices(only_updated=True))
        nv = self.nvox
        out = {"indices": np.zeros((max(n, 1), 3), np.int32), "distance": np.empty((max(n, 1), nv), np.float32),
               "weight": np.empty((max(n, 1), nv), np.float32), "color": np.empty((max(n, 1), nv, 4), np.uint8),
               "last_observed": np.empty((max(n, 1), nv), np.uint64), "flags": np.empty((max(n, 1), nv), np.uint8),
               "sem_label": np.empty((max(n, 1), nv), np.uint32)}
        k = self._chk(self.lib.khr_download_updated(self.h, _ptr(out["indices"]), _ptr(out["distance"]), _ptr(out["weight"]),
                                                    _ptr(out["color"]), _ptr(out["last_observed"]), _ptr(out["flags"]),
                                                    _ptr(out["sem_label"]), max(n, 1)))
        return {a: b[:k] for a, b in out.items()}

    def snapshot_updated(self, fields=63, cap_blocks=0):
        """VolumetricMap::cloneUpdated with snapshot semantics: a device-side copy that outlives later map changes."""
        h = C.c_void_p()
        self._chk(self.lib.khr_snapshot_updated(self.h, int(fields), int(cap_blocks), C.byref(h)))
        return Snapshot(self, h)

    def take_snapshot(self):
        """the snapshot queued by process_frame(.. PF_SNAPSHOT | PF_OUTPUT ..), or None"""
        h = C.c_void_p()
        rc = self.lib.khr_take_snapshot(self.h, C.byref(h))
        return Snapshot(self, h) if rc == 0 and h.value else None

    def reserve_mesh_staging(self, n_vertices):
        """room for n_vertices in the pinned block behind fetch_mesh, allocated now instead of by growth in the middle of a run"""
        self._chk(self.lib.khr_reserve_mesh_staging(self.h, int(n_vertices)))

    def reserve_snapshots(self, n, fields=63, cap_blocks=0):
        """n snapshot arenas allocated now (a snapshot that finds none free allocates one in the middle of the run)"""
        self._chk(self.lib.khr_reserve_snapshots(self.h, int(fields), int(cap_blocks), int(n)))

    def download_mesh(self):
        n = self._chk(self.lib.khr_mesh_num_vertices(self.h))
        pts = np.empty((max(n, 1), 3), np.float32)
        col = np.empty((max(n, 1), 4), np.uint8)
        lab = np.empty(max(n, 1), np.uint32)
        fs = np.empty(max(n, 1), np.uint64)
        st = np.empty(max(n, 1), np.uint64)
        k = self._chk(self.lib.khr_download_mesh(self.h, _ptr(pts), _ptr(col), _ptr(lab), _ptr(fs), _ptr(st), max(n, 1)))
        return {"points": pts[:k], "colors": col[:k], "labels": lab[:k], "first_seen": fs[:k], "stamps": st[:k]}

    def fetch_mesh_launch(self):
        """queue the gather of the current mesh; the next fetch_mesh() only collects it"""
        self._chk(self.lib.khr_fetch_mesh_launch(self.h))

    def fetch_mesh(self):
        """the same mesh through khr_fetch_mesh / khr_fetch_mesh_into (one host round trip)."""
        v = C.c_int64(0)
        n = self._chk(self.lib.khr_fetch_mesh(self.h, C.byref(v)))
        pts = np.empty((n, 3), np.float32)
        col = np.empty((n, 4), np.uint8)
        lab = np.empty(n, np.uint32)
        fs = np.empty(n, np.uint64)
        st = np.empty(n, np.uint64)
        if n:
            self._chk(self.lib.khr_fetch_mesh_into(self.h, _ptr(pts), _ptr(col), _ptr(lab), _ptr(fs), _ptr(st)))
        return {"points": pts, "colors": col, "labels": lab, "first_seen": fs, "stamps": st}

    WELD_FIELDS = (("points", np.float32, (3,), "v"), ("colors", np.uint8, (4,), "v"), ("labels", np.uint32, (), "v"),
                   ("first_seen", np.uint64, (), "v"), ("stamps", np.uint64, (), "v"), ("faces", np.uint32, (3,), "f"),
                   ("soup_to_vertex", np.uint32, (), "s"))

    def weld_mesh_into(self, out, on_device=False):
        """khr_weld_mesh_into: the result of the last weld into caller buffers (`out`: WELD_FIELDS name -> contiguous array, or an
        integer device pointer with on_device; absent / None = not copied).  Returns the return code without raising."""
        ptrs = []
        for name, _, _, _ in self.WELD_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_weld_mesh_into(self.h, int(on_device), *ptrs)

    def weld_mesh(self, resolution, device=False):
        """The mesh of the last generate_mesh as an indexed mesh, welded on the device at `resolution` metres (khr_weld_mesh,
        ASSUMPTIONS.md A.16).  Returns a dict: points (n, 3) float32, colors (n, 4) uint8, labels (n,) uint32, first_seen / stamps
        (n,) uint64 of the welded vertices, faces (m, 3) uint32, soup_to_vertex (n_soup,) uint32, and stats (n_soup_vertices,
        n_vertices, n_faces, n_degenerate_faces).  device=True: torch tensors on the context's device (int32 / int64 stand in for the
        unsigned types), copied device to device and complete when the call returns."""
        st = KhrWeldStats()
        self._chk(self.lib.khr_weld_mesh(self.h, float(resolution), C.byref(st)))
        stats = {k: int(getattr(st, k)) for k, _ in KhrWeldStats._fields_}
        n = {"v": stats["n_vertices"], "f": stats["n_faces"], "s": stats["n_soup_vertices"]}
        if device:
            import torch
            dev = torch.device("cuda", self.cfg.device)
            tdt = {np.float32: torch.float32, np.uint8: torch.uint8, np.uint32: torch.int32, np.uint64: torch.int64}
            out = {k: torch.empty((n[w],) + sh, dtype=tdt[dt], device=dev) for k, dt, sh, w in self.WELD_FIELDS}
            self._chk(self.weld_mesh_into({k: t.data_ptr() for k, t in out.items()}, on_device=True))
            self.sync()  # (the copies ran on the context's stream: complete before torch reads the tensors on its own)
        else:
            out = {k: np.zeros((n[w],) + sh, dt) for k, dt, sh, w in self.WELD_FIELDS}
            self._chk(self.weld_mesh_into(out))
        out["stats"] = stats
        return out

    @staticmethod
    def merge_request(mode, voxel_offset=(0, 0, 0), pose=None, min_weight=0.0):
        """khr_merge_request: mode KHR_MERGE_ALIGNED with an integer voxel offset, or KHR_MERGE_RESAMPLE with `pose` = dst_T_src
        (4x4, rigid); min_weight 0 = the destination's mesh_min_weight"""
        rq = KhrMergeRequest()
        rq.mode = int(mode)
        rq.voxel_offset[:] = [int(v) for v in voxel_offset]
        rq.dst_T_src[:] = np.asarray(np.eye(4) if pose is None else pose, np.float64).reshape(16).tolist()
        rq.min_weight = float(min_weight)
        return rq

    def merge_map_rc(self, src, request):
        """khr_merge_map without raising: (return code, statistics dict)"""
        st = KhrMergeStats()
        rc = self.lib.khr_merge_map(self.h, src.h if src is not None else None, C.byref(request) if request is not None else None, C.byref(st))
        return rc, {k: int(getattr(st, k)) for k, _ in KhrMergeStats._fields_}

    def merge_map(self, src, mode=KHR_MERGE_ALIGNED, voxel_offset=(0, 0, 0), pose=None, min_weight=0.0, request=None):
        """Fuse the map of the context `src` into this one on the device (khr_merge_map, ASSUMPTIONS.md A.17); `src` is only
        read.  Returns the statistics as a dict."""
        rq = request if request is not None else self.merge_request(mode, voxel_offset, pose, min_weight)
        rc, st = self.merge_map_rc(src, rq)
        self._chk(rc)
        return st

    DIFF_FIELDS = (("voxels", np.int32, (3,), "v"), ("kind", np.uint8, (), "v"), ("d_now", np.float32, (), "v"), ("d_then", np.float32, (), "v"),
                   ("label", np.uint32, (), "v"), ("stamp_now", np.uint64, (), "v"), ("stamp_then", np.uint64, (), "v"),
                   ("blocks", np.int32, (3,), "b"), ("block_appeared", np.uint32, (), "b"), ("block_disappeared", np.uint32, (), "b"),
                   ("block_first", np.uint32, (), "b"))

    def diff_request(self, mode=KHR_MERGE_ALIGNED, voxel_offset=(0, 0, 0), pose=None, min_weight=0.0, occupied_distance=None, free_distance=None):
        """khr_diff_request: mode / voxel_offset / pose (= ctx_T_ref) / min_weight as in merge_request; occupied_distance defaults to
        0 and free_distance to this context's voxel_size"""
        rq = KhrDiffRequest()
        rq.mode = int(mode)
        rq.voxel_offset[:] = [int(v) for v in voxel_offset]
        rq.ctx_T_ref[:] = np.asarray(np.eye(4) if pose is None else pose, np.float64).reshape(16).tolist()
        rq.min_weight = float(min_weight)
        rq.occupied_distance = 0.0 if occupied_distance is None else float(occupied_distance)
        rq.free_distance = float(self.cfg.voxel_size) if free_distance is None else float(free_distance)
        return rq

    def diff_map_rc(self, ref, request):
        """khr_diff_map without raising: (return code, statistics dict)"""
        st = KhrDiffStats()
        rc = self.lib.khr_diff_map(self.h, ref.h if ref is not None else None, C.byref(request) if request is not None else None, C.byref(st))
        return rc, {k: int(getattr(st, k)) for k, _ in KhrDiffStats._fields_}

    def diff_map_into(self, out, on_device=False):
        """khr_diff_map_into: the result of the last diff into caller buffers (`out`: DIFF_FIELDS name -> contiguous array, or an
        integer device pointer with on_device; absent / None = not copied).  Returns the return code without raising."""
        ptrs = []
        for name, _, _, _ in self.DIFF_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_diff_map_into(self.h, int(on_device), *ptrs)

    def diff_map(self, ref, mode=KHR_MERGE_ALIGNED, voxel_offset=(0, 0, 0), pose=None, min_weight=0.0, occupied_distance=None, free_distance=None,
                 request=None):
        """The voxels that appeared or vanished in this context's map against the map of the context `ref`, found on the device
        (khr_diff_map, ASSUMPTIONS.md A.18); neither map is written.  `ref` is sampled as merge_map samples its source (mode,
        voxel_offset, pose = ctx_T_ref, min_weight).  A compared voxel appeared iff d_then >= free_distance and d_now <=
        occupied_distance, and disappeared iff d_then <= occupied_distance and d_now >= free_distance; the defaults are
        occupied_distance = 0 and free_distance = voxel_size.  Returns a dict: the statistics under "stats", per changed voxel
        voxels (n, 3) int32, kind uint8 (1 appeared, 2 disappeared), d_now / d_then float32, label uint32, stamp_now / stamp_then
        uint64, per changed block blocks (m, 3) int32, block_appeared / block_disappeared / block_first uint32 -- blocks in (x, y, z)
        order, the voxels of a block in ascending linear index."""
        rq = request if request is not None else self.diff_request(mode, voxel_offset, pose, min_weight, occupied_distance, free_distance)
        rc, stats = self.diff_map_rc(ref, rq)
        self._chk(rc)
        n = {"v": stats["n_appeared"] + stats["n_disappeared"], "b": stats["n_changed_blocks"]}
        out = {k: np.zeros((n[w],) + sh, dt) for k, dt, sh, w in self.DIFF_FIELDS}
        self._chk(self.diff_map_into(out))
        out["stats"] = stats
        return out

    SEGMENT_FIELDS = (("label", np.int32, (), "c"), ("n_voxels", np.uint64, (), "c"), ("bbox_min", np.int32, (3,), "c"), ("bbox_max", np.int32, (3,), "c"),
                      ("sum", np.int64, (3,), "c"), ("representative", np.int32, (3,), "c"), ("last_observed_max", np.uint64, (), "c"),
                      ("first", np.uint64, (), "c"), ("voxels", np.int32, (3,), "v"), ("voxel_component", np.uint32, (), "v"))

    def segment_request(self, min_weight=0.0, surface_distance=0.0, connectivity=26, by_label=None, labels=None, flags_require=0, flags_exclude=0,
                        min_voxels=1, max_voxels=0, want_voxels=True):
        """khr_segment_request: min_weight 0 = this context's mesh_min_weight; by_label defaults to True when the context has
        semantics; labels None / empty = every label; max_voxels <= 0 = unlimited.  The request keeps its label array alive."""
        rq = KhrSegmentRequest()
        rq.min_weight, rq.surface_distance = float(min_weight), float(surface_distance)
        rq.connectivity = int(connectivity)
        rq.by_label = int(bool(self.cfg.with_semantics) if by_label is None else bool(by_label))
        lab = [] if labels is None else [int(v) for v in labels]
        rq._labels = (C.c_int32 * max(1, len(lab)))(*lab)
        rq.labels = C.cast(rq._labels, C.POINTER(C.c_int32)) if lab else None
        rq.n_labels = len(lab)
        rq.flags_require, rq.flags_exclude = int(flags_require), int(flags_exclude)
        rq.min_voxels, rq.max_voxels = int(min_voxels), int(max_voxels)
        rq.want_voxels = int(bool(want_voxels))
        return rq

    def segment_map_rc(self, request):
        """khr_segment_map without raising: (return code, statistics dict)"""
        st = KhrSegmentStats()
        rc = self.lib.khr_segment_map(self.h, C.byref(request) if request is not None else None, C.byref(st))
        return rc, {k: int(getattr(st, k)) for k, _ in KhrSegmentStats._fields_}

    def segment_map_into(self, out, on_device=False):
        """khr_segment_map_into: the result of the last segmentation into caller buffers (`out`: SEGMENT_FIELDS name -> contiguous
        array, or an integer device pointer with on_device; absent / None = not copied).  Returns the return code without raising."""
        ptrs = []
        for name, _, _, _ in self.SEGMENT_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_segment_map_into(self.h, int(on_device), *ptrs)

    def segment_map(self, request=None, **kw):
        """The connected components of this context's occupied voxels, found on the device (khr_segment_map, ASSUMPTIONS.md A.19);
        the map is not written.  Keywords as segment_request.  Returns a dict: the statistics under "stats", per kept component
        label int32, n_voxels uint64, bbox_min / bbox_max (m, 3) int32 (global voxel indices, inclusive), sum (m, 3) int64,
        representative (m, 3) int32, last_observed_max uint64, first uint64 and centroid (m, 3) float64 in metres; with
        want_voxels also voxels (n, 3) int32 and voxel_component uint32 (ids from 1), grouped by component in ascending id."""
        rq = request if request is not None else self.segment_request(**kw)
        rc, stats = self.segment_map_rc(rq)
        self._chk(rc)
        n = {"c": stats["n_components"], "v": stats["n_voxels"]}
        out = {k: np.zeros((n[w],) + sh, dt) for k, dt, sh, w in self.SEGMENT_FIELDS if w == "c" or rq.want_voxels}
        self._chk(self.segment_map_into(out))
        out["centroid"] = (out["sum"].astype(np.float64) / np.maximum(out["n_voxels"], 1).astype(np.float64)[:, None] + 0.5) * float(self.cfg.voxel_size)
        out["stats"] = stats
        return out

    # name, dtype, trailing shape, "d" = one entry per cell of the box / "l" = one per listed cell
    VOR_FIELDS = (("distance", np.float32, (), "d"), ("d2", np.int32, (), "d"), ("status", np.uint8, (), "d"), ("site", np.int32, (), "d"),
                  ("basis", np.uint8, (), "d"), ("cells", np.int32, (3,), "l"), ("cell_distance", np.float32, (), "l"),
                  ("cell_basis", np.uint8, (), "l"), ("cell_sites", np.int32, (KHR_VOR_MAX_BASIS, 3), "l"))

    @staticmethod
    def voronoi_request(origin, dims, ratio=1, max_distance=1.0, min_weight=0.0, surface_distance=0.0, unknown_is_obstacle=False,
                        min_distance=0.0, mode=KHR_VOR_L1_THEN_ANGLE, parent_l1_separation=20, parent_cos_angle_separation=0.2, min_basis=2):
        """a khr_voronoi_request: `origin` (first cell) and `dims` (cells per axis) as x, y, z"""
        rq = KhrVoronoiRequest()
        for a in range(3):
            rq.origin[a], rq.dims[a] = int(origin[a]), int(dims[a])
        rq.ratio = int(ratio)
        rq.min_weight, rq.max_distance, rq.surface_distance = float(min_weight), float(max_distance), float(surface_distance)
        rq.unknown_is_obstacle = int(bool(unknown_is_obstacle))
        rq.min_distance, rq.mode, rq.parent_l1_separation = float(min_distance), int(mode), int(parent_l1_separation)
        rq.parent_cos_angle_separation, rq.min_basis = float(parent_cos_angle_separation), int(min_basis)
        return rq

    def voronoi_field_rc(self, request):
        """khr_voronoi_field without raising: (return code, statistics dict)"""
        st = KhrVoronoiStats()
        rc = self.lib.khr_voronoi_field(self.h, C.byref(request) if request is not None else None, C.byref(st))
        return rc, {k: int(getattr(st, k)) for k, _ in KhrVoronoiStats._fields_}

    def voronoi_field_into(self, out, on_device=False):
        """khr_voronoi_field_into: the result of the last Voronoi field into caller buffers (`out`: VOR_FIELDS name -> contiguous
        array, or an integer device pointer with on_device; absent / None = not copied).  Returns the return code without raising."""
        ptrs = []
        for name, _, _, _ in self.VOR_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_voronoi_field_into(self.h, int(on_device), *ptrs)

    def voronoi_field(self, origin, dims, ratio=1, max_distance=1.0, request=None, **kw):
        """The nearest obstacle cell and the generalized Voronoi cells of a box of the live map (khr_voronoi_field, ASSUMPTIONS.md
        A.20); the map is not written.  Keywords as voronoi_request.  Returns a dict: distance float32, d2 int32, status uint8 (those
        of distance_field(positive_only=True)), site int32 (the linear index x + nx * (y + ny * z) of the nearest obstacle cell, -1
        without one) and basis uint8, shaped (nz, ny, nx); the list of the cells with basis >= min_basis in ascending linear index:
        cells (m, 3) int32 global cell indices, cell_distance float32, cell_basis uint8, cell_sites (m, 4, 3) int32 (unused entries
        zero); cell_size; and stats."""
        rq = request if request is not None else self.voronoi_request(origin, dims, ratio, max_distance, **kw)
        rc, stats = self.voronoi_field_rc(rq)
        self._chk(rc)
        shape = {"d": (int(rq.dims[2]), int(rq.dims[1]), int(rq.dims[0])), "l": (stats["n_listed"],)}
        out = {k: np.zeros(shape[w] + sh, dt) for k, dt, sh, w in self.VOR_FIELDS}
        self._chk(self.voronoi_field_into(out))
        out["cell_size"] = float(np.float32(self.cfg.voxel_size) * np.float32(int(rq.ratio)))
        out["stats"] = stats
        return out

    # name, dtype, trailing shape, "d" = one entry per cell of the box / "p" = one per kept place / "e" = one per kept edge
    PL_FIELDS = (("place", np.int32, (), "d"), ("centre", np.int32, (3,), "p"), ("centre_d2", np.int32, (), "p"), ("radius", np.float32, (), "p"),
                 ("basis", np.uint8, (), "p"), ("site", np.int32, (3,), "p"), ("n_cells", np.uint32, (), "p"), ("sum", np.int64, (3,), "p"),
                 ("degree", np.uint32, (), "p"), ("component", np.uint32, (), "p"), ("edge_a", np.uint32, (), "e"), ("edge_b", np.uint32, (), "e"),
                 ("edge_clearance_d2", np.int32, (), "e"), ("edge_n_contacts", np.uint32, (), "e"))
    PL_INPUTS = (("distance", np.float32), ("d2", np.int32), ("basis", np.uint8), ("site", np.int32))

    @staticmethod
    def places_request(min_basis=0, min_node_distance=0.0, compression=4, min_component_size=1):
        """a khr_places_request"""
        rq = KhrPlacesRequest()
        rq.min_basis, rq.min_node_distance, rq.compression, rq.min_component_size = int(min_basis), float(min_node_distance), int(compression), int(min_component_size)
        return rq

    def places_graph_rc(self, request):
        """khr_places_graph without raising: (return code, statistics dict)"""
        st = KhrPlacesStats()
        rc = self.lib.khr_places_graph(self.h, C.byref(request) if request is not None else None, C.byref(st))
        if rc == 0:
            self._places_kept = int(st.n_places)  # (travel_field(goals="places") sizes its goals with it)
        return rc, {k: int(getattr(st, k)) for k, _ in KhrPlacesStats._fields_}

    def places_graph_from_rc(self, request, origin, dims, field, on_device=False):
        """khr_places_graph_from without raising: (return code, statistics dict).  `field`: PL_INPUTS name -> contiguous array of
        the box's cells, or an integer device pointer with on_device; origin / dims / an input may be None (an argument error)"""
        st = KhrPlacesStats()
        o = None if origin is None else (C.c_int32 * 3)(*[int(v) for v in origin])
        d = None if dims is None else (C.c_int32 * 3)(*[int(v) for v in dims])
        ptrs, keep = [], []
        for name, dt in self.PL_INPUTS:
            a = field.get(name)
            if a is None:
                ptrs.append(None)
            elif on_device:
                ptrs.append(C.c_void_p(int(a)))
            else:
                a = np.ascontiguousarray(a, dt)
                keep.append(a)
                ptrs.append(_ptr(a))
        rc = self.lib.khr_places_graph_from(self.h, C.byref(request) if request is not None else None, o, d, int(on_device), *ptrs, C.byref(st))
        if rc == 0:
            self._places_kept = int(st.n_places)
        return rc, {k: int(getattr(st, k)) for k, _ in KhrPlacesStats._fields_}

    def places_graph_into(self, out, on_device=False):
        """khr_places_graph_into: the result of the last places graph into caller buffers (`out`: PL_FIELDS name -> contiguous array,
        or an integer device pointer with on_device; absent / None = not copied).  Returns the return code without raising."""
        ptrs = []
        for name, _, _, _ in self.PL_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_places_graph_into(self.h, int(on_device), *ptrs)

    def places_graph_box(self):
        """khr_places_graph_box: (origin, dims) of the box the last places graph describes, as x, y, z"""
        o, d = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        self._chk(self.lib.khr_places_graph_box(self.h, o, d))
        return tuple(int(v) for v in o), tuple(int(v) for v in d)

    def _places_result(self, stats):
        dims = self.places_graph_box()[1]
        shape = {"d": (int(dims[2]), int(dims[1]), int(dims[0])), "p": (stats["n_places"],), "e": (stats["n_edges"],)}
        out = {k: np.zeros(shape[w] + sh, dt) for k, dt, sh, w in self.PL_FIELDS}
        self._chk(self.places_graph_into(out))
        out["centroid"] = out["sum"].astype(np.float64) / np.maximum(out["n_cells"], 1).astype(np.float64)[:, None]
        out["stats"] = stats
        return out

    def places_graph(self, min_basis=0, min_node_distance=0.0, compression=4, min_component_size=1):
        """The places and their links from the last voronoi_field of this context (khr_places_graph, ASSUMPTIONS.md A.21).  Returns a
        dict: place int32 (nz, ny, nx) over that field's box, the kept place of a member cell or -1; per kept place centre (p, 3)
        int32 global cell, centre_d2, radius float32, basis, site (p, 3), n_cells, sum (p, 3) int64, centroid (p, 3) float64 =
        sum / n_cells, degree, component; per kept edge edge_a < edge_b, edge_clearance_d2, edge_n_contacts; and stats."""
        rc, stats = self.places_graph_rc(self.places_request(min_basis, min_node_distance, compression, min_component_size))
        self._chk(rc)
        return self._places_result(stats)

    def places_graph_from(self, origin, dims, distance, d2, basis, site, min_basis=0, min_node_distance=0.0, compression=4, min_component_size=1,
                          on_device=False):
        """places_graph on a field the caller brings (khr_places_graph_from): the box and four arrays of its cells in the order
        x + nx * (y + ny * z) -- numpy arrays, or integer device pointers with on_device"""
        rq = self.places_request(min_basis, min_node_distance, compression, min_component_size)
        rc, stats = self.places_graph_from_rc(rq, origin, dims, dict(distance=distance, d2=d2, basis=basis, site=site), on_device)
        self._chk(rc)
        return self._places_result(stats)

    # name, dtype of the per-cell results of a travel field; of the per-start results of its paths
    TF_FIELDS = (("cost", np.uint32), ("goal", np.int32), ("parent", np.uint8))
    TF_INPUTS = (("distance", np.float32), ("status", np.uint8))

    @staticmethod
    def travel_request(clearance=0.0, connectivity=26, allow_unknown=False, max_cost=0):
        """a khr_travel_request"""
        rq = KhrTravelRequest()
        rq.clearance, rq.connectivity, rq.allow_unknown, rq.max_cost = float(clearance), int(connectivity), int(bool(allow_unknown)), int(max_cost)
        return rq

    @staticmethod
    def _travel_goals(goals, on_device, n_goals):
        """(pointer, count, what to keep alive) of a goal list: an (n, 3) array, or an integer device pointer with n_goals"""
        if goals is None:
            return None, 0 if n_goals is None else int(n_goals), None
        if on_device:
            return C.c_void_p(int(goals)), int(n_goals), None
        g = np.ascontiguousarray(goals, np.int32).reshape(-1, 3)
        return _ptr(g), (len(g) if n_goals is None else int(n_goals)), g

    def travel_field_rc(self, request, goals, goals_on_device=False, n_goals=None):
        """khr_travel_field without raising: (return code, statistics dict)"""
        st = KhrTravelStats()
        gp, n, keep = self._travel_goals(goals, goals_on_device, n_goals)
        rc = self.lib.khr_travel_field(self.h, C.byref(request) if request is not None else None, gp, n, int(goals_on_device), C.byref(st))
        return rc, {k: int(getattr(st, k)) for k, _ in KhrTravelStats._fields_}

    def travel_field_from_rc(self, request, origin, dims, field, goals, on_device=False, n_goals=None):
        """khr_travel_field_from without raising: (return code, statistics dict).  `field`: TF_INPUTS name -> contiguous array of the
        box's cells, or an integer device pointer with on_device (then `goals` is one too, with n_goals); origin / dims / an input /
        goals may be None (an argument error)"""
        st = KhrTravelStats()
        o = None if origin is None else (C.c_int32 * 3)(*[int(v) for v in origin])
        d = None if dims is None else (C.c_int32 * 3)(*[int(v) for v in dims])
        ptrs, keep = [], []
        for name, dt in self.TF_INPUTS:
            a = field.get(name)
            if a is None:
                ptrs.append(None)
            elif on_device:
                ptrs.append(C.c_void_p(int(a)))
            else:
                a = np.ascontiguousarray(a, dt)
                keep.append(a)
                ptrs.append(_ptr(a))
        gp, n, g = self._travel_goals(goals, on_device, n_goals)
        rc = self.lib.khr_travel_field_from(self.h, C.byref(request) if request is not None else None, o, d, int(on_device), *ptrs, gp, n, C.byref(st))
        return rc, {k: int(getattr(st, k)) for k, _ in KhrTravelStats._fields_}

    def travel_field_into(self, out, on_device=False):
        """khr_travel_field_into: the last travel field into caller buffers (`out`: TF_FIELDS name -> contiguous array, or an integer
        device pointer with on_device; absent / None = not copied).  Returns the return code without raising."""
        ptrs = []
        for name, _ in self.TF_FIELDS:
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_travel_field_into(self.h, int(on_device), *ptrs)

    def travel_field_box(self):
        """khr_travel_field_box: (origin, dims) of the box the last travel field describes, as x, y, z"""
        o, d = (C.c_int32 * 3)(), (C.c_int32 * 3)()
        self._chk(self.lib.khr_travel_field_box(self.h, o, d))
        return tuple(int(v) for v in o), tuple(int(v) for v in d)

    def _travel_result(self, stats):
        origin, dims = self.travel_field_box()
        shape = (int(dims[2]), int(dims[1]), int(dims[0]))
        out = {k: np.zeros(shape, dt) for k, dt in self.TF_FIELDS}
        self._chk(self.travel_field_into(out))
        out["origin"], out["dims"], out["stats"] = origin, dims, stats
        return out

    def places_centres(self):
        """the centres (p, 3) int32, global cells, of the kept places of the last places graph, in place order"""
        p = getattr(self, "_places_kept", None)
        centre = np.zeros((0 if p is None else p, 3), np.int32)
        self._chk(self.places_graph_into({"centre": centre}))  # (KHR_ESTATE without a graph)
        return centre

    def travel_field(self, goals, clearance, connectivity=26, allow_unknown=False, max_cost=0, field=None):
        """Travel cost to the nearest goal by travel, for a body of radius `clearance` metres (khr_travel_field, ASSUMPTIONS.md A.22),
        over the box of the last voronoi_field of this context -- or over `field` = (origin, dims, distance, status), arrays of the
        box's cells as distance_field / voronoi_field return them (khr_travel_field_from).  `goals`: (n, 3) global cells, or
        "places": the centres of the kept places of the last places graph, in place order, so that `goal` says to which place a cell
        belongs by travel.  Returns a dict: cost uint32 (nz, ny, nx), KHR_TF_UNREACHED where no goal reaches; goal int32, -1 there;
        parent uint8, the code of the next cell towards the goal (13 at a goal, 255 unreached); origin, dims; stats."""
        if isinstance(goals, str):
            if goals != "places":
                raise ValueError("goals: an (n, 3) array of cells or \"places\"")
            goals = self.places_centres()
        rq = self.travel_request(clearance, connectivity, allow_unknown, max_cost)
        if field is None:
            rc, stats = self.travel_field_rc(rq, goals)
        else:
            origin, dims, distance, status = field
            rc, stats = self.travel_field_from_rc(rq, origin, dims, dict(distance=distance, status=status), goals)
        self._chk(rc)
        return self._travel_result(stats)

    def travel_paths_rc(self, starts, on_device=False, n_starts=None):
        """khr_travel_paths without raising: (return code, cells in all paths)"""
        total = C.c_uint64(0)
        sp, n, keep = self._travel_goals(starts, on_device, n_starts)
        rc = self.lib.khr_travel_paths(self.h, n, sp, int(on_device), C.byref(total))
        if rc == 0:
            self._travel_paths_shape = (n, int(total.value))
        return rc, int(total.value)

    def travel_paths_into(self, out, on_device=False):
        """khr_travel_paths_into: offsets / cells / path_cost / path_goal of the last travel_paths into caller buffers"""
        ptrs = []
        for name in ("offsets", "cells", "path_cost", "path_goal"):
            a = out.get(name)
            ptrs.append(None if a is None else (C.c_void_p(int(a)) if on_device else _ptr(a)))
        return self.lib.khr_travel_paths_into(self.h, int(on_device), *ptrs)

    def travel_paths(self, starts):
        """The paths from `starts` ((n, 3) global cells) to their goals through the last travel field (khr_travel_paths).  Returns a
        dict: offsets int64 (n + 1), cells (total, 3) int32 global cells -- path i is cells[offsets[i]:offsets[i + 1]], start and
        goal included, empty for a start outside the box or unreached --, path_cost uint32, path_goal int32, and paths, the list of
        the per-start slices of cells."""
        rc, total = self.travel_paths_rc(starts)
        self._chk(rc)
        n = self._travel_paths_shape[0]
        out = {"offsets": np.zeros(n + 1, np.int64), "cells": np.zeros((total, 3), np.int32), "path_cost": np.zeros(n, np.uint32), "path_goal": np.zeros(n, np.int32)}
        self._chk(self.travel_paths_into(out))
        out["paths"] = [out["cells"][out["offsets"][i]:out["offsets"][i + 1]] for i in range(n)]
        return out

    def fetch_mesh_reuse(self, bufs):
        """fetch_mesh() into arrays the caller keeps (a consumer that takes one mesh per output must not pay page faults on 20 MB of
        fresh arrays every time): `bufs` = dict, grown when the mesh outgrows it -> vertex count"""
        v = C.c_int64(0)
        n = self._chk(self.lib.khr_fetch_mesh(self.h, C.byref(v)))
        if n > bufs.get("cap", 0):
            cap = int(n * 1.5) + 1024
            bufs.update(cap=cap, points=np.empty((cap, 3), np.float32), colors=np.empty((cap, 4), np.uint8), labels=np.empty(cap, np.uint32),
                        first_seen=np.empty(cap, np.uint64), stamps=np.empty(cap, np.uint64))
            for k in ("points", "colors", "labels", "first_seen", "stamps"):
                bufs[k].fill(0)  # touch the pages now
        if n:
            self._chk(self.lib.khr_fetch_mesh_into(self.h, _ptr(bufs["points"]), _ptr(bufs["colors"]), _ptr(bufs["labels"]), _ptr(bufs["first_seen"]),
                                                   _ptr(bufs["stamps"])))
        return n

    def timing_enable(self, on=True, names=None):
        """on=True: all timers, or only those in `names`."""
        mask = 0
        if on:
            mask = 0xFF if names is None else sum(1 << self.TIMERS[n] for n in names)
        self._chk(self.lib.khr_timing_enable(self.h, mask))

    def timing_reset(self):
        self._chk(self.lib.khr_timing_reset(self.h))

    def timing_get(self, name):
        ms, n = C.c_double(0), C.c_uint64(0)
        self._chk(self.lib.khr_timing_get(self.h, self.TIMERS[name], C.byref(ms), C.byref(n)))
        return ms.value, n.value


class Snapshot:
    """khr_snapshot: the updated blocks as they were when the snapshot was taken (ActiveWindowOutput::map role)."""

    def __init__(self, ctx, handle):
        self.ctx, self.h = ctx, handle

    def num_blocks(self):
        return self.ctx._chk(self.ctx.lib.khr_snapshot_num_blocks(self.h))

    def download(self):
        n = max(1, self.num_blocks())
        nv = self.ctx.nvox
        out = {"indices": np.zeros((n, 3), np.int32), "distance": np.empty((n, nv), np.float32),
               "weight": np.empty((n, nv), np.float32), "color": np.empty((n, nv, 4), np.uint8),
               "last_observed": np.zeros((n, nv), np.uint64), "flags": np.empty((n, nv), np.uint8),
               "sem_label": np.zeros((n, nv), np.uint32)}
        k = self.ctx._chk(self.ctx.lib.khr_snapshot_download(self.h, _ptr(out["indices"]), _ptr(out["distance"]), _ptr(out["weight"]),
                                                             _ptr(out["color"]), _ptr(out["last_observed"]), _ptr(out["flags"]),
                                                             _ptr(out["sem_label"]), n))
        # the C ABI hands the blocks out in the snapshot's own order; sorted by block index here (tests, small maps)
        order = np.lexsort((out["indices"][:k, 2], out["indices"][:k, 1], out["indices"][:k, 0]))
        return {a: b[:k][order] for a, b in out.items()}

    def download_extra(self, num_labels):
        """the optional fields (KHR_SNAP_LAST_OCCUPIED = 64, KHR_SNAP_LIKELIHOODS = 128), blocks sorted by index"""
        n = max(1, self.num_blocks())
        nv = self.ctx.nvox
        out = {"indices": np.zeros((n, 3), np.int32), "last_occupied": np.zeros((n, nv), np.uint64),
               "likelihoods": np.zeros((n, nv, num_labels), np.float32)}
        k = self.ctx._chk(self.ctx.lib.khr_snapshot_download_extra(self.h, _ptr(out["indices"]), _ptr(out["last_occupied"]),
                                                                   _ptr(out["likelihoods"]), n))
        order = np.lexsort((out["indices"][:k, 2], out["indices"][:k, 1], out["indices"][:k, 0]))
        return {a: b[:k][order] for a, b in out.items()}

    def download_into(self, ptrs, cap_blocks):
        """raw form: `ptrs` = 7 host addresses (indices, distance, weight, colour, last_observed, flags, label; 0 = skip),
        e.g. of pinned buffers; blocks in the snapshot's own order.  -> block count"""
        return self.ctx._chk(self.ctx.lib.khr_snapshot_download(self.h, *[C.c_void_p(p or None) for p in ptrs], int(cap_blocks)))

    def poll(self):
        """non-blocking: True once the block count is known"""
        return self.ctx._chk(self.ctx.lib.khr_snapshot_poll(self.h)) == 1

    def download_begin(self, ptrs, cap_blocks):
        """asynchronous download_into (khr_snapshot_download_begin): the copies run on the context's copy stream beside the next
        frames' kernels; non-zero entries of `ptrs` are the consumer's field mask.  download_end() waits and returns the count"""
        self.ctx._chk(self.ctx.lib.khr_snapshot_download_begin(self.h, *[C.c_void_p(p or None) for p in ptrs], int(cap_blocks)))

    def download_end(self):
        return self.ctx._chk(self.ctx.lib.khr_snapshot_download_end(self.h))

    def release(self):
        if self.h is not None and self.h.value:
            self.ctx.lib.khr_snapshot_release(self.h)
        self.h = None


class RayVerificator:
    """ctypes wrapper of the khr_rv_* calls (khronos::RayVerificator on the device)."""

    def __init__(self, block_size=1.0, radial_tolerance=0.1, depth_tolerance=0.1, device=0):
        self.lib = load_library()
        self.h = C.c_void_p()
        rc = self.lib.khr_rv_create(float(block_size), float(radial_tolerance), float(depth_tolerance), int(device), C.byref(self.h))
        if rc < 0:
            raise KhronosAmdError("khr_rv_create failed (%d): %s" % (rc, self.lib.khr_last_error().decode()))

    def close(self):
        if self.h:
            self.lib.khr_rv_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc < 0:
            raise KhronosAmdError("khr_rv call failed (%d): %s" % (rc, self.lib.khr_last_error().decode()))
        return rc

    def clear(self):
        self._chk(self.lib.khr_rv_clear(self.h))

    def add_rays(self, stamps, sources, targets):
        st = np.ascontiguousarray(stamps, dtype=np.uint64)
        sr = np.ascontiguousarray(sources, dtype=np.float32).reshape(-1, 3)
        tg = np.ascontiguousarray(targets, dtype=np.float32).reshape(-1, 3)
        assert st.size == sr.shape[0] == tg.shape[0]
        self._chk(self.lib.khr_rv_add_rays(self.h, st.size, _ptr(st), _ptr(sr), _ptr(tg)))

    def num_rays(self):
        return self._chk(self.lib.khr_rv_num_rays(self.h))

    def num_pairs(self):
        return self._chk(self.lib.khr_rv_num_pairs(self.h))

    def check(self, points, earliest, latest):
        """-> (n_present[m], n_absent[m], present_stamps, absent_stamps); stamps grouped by point in query order."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        m = pts.shape[0]
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(earliest, np.uint64), (m,)))
        t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(latest, np.uint64), (m,)))
        npres, nabs = np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
        tp, ta = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.khr_rv_check(self.h, m, _ptr(pts), _ptr(t0), _ptr(t1), _ptr(npres), _ptr(nabs), C.byref(tp), C.byref(ta)))
        pres, absn = np.zeros(max(tp.value, 1), np.uint64), np.zeros(max(ta.value, 1), np.uint64)
        if m:
            self._chk(self.lib.khr_rv_check_stamps(self.h, _ptr(pres), _ptr(absn)))
        return npres[:m], nabs[:m], pres[:tp.value], absn[:ta.value]

    def check_and_vote(self, points, earliest, latest, forward, temporal_resolution=1.0, window_size=5,
                       use_relative_confidence=True, absence_confidence=0.5, presence_confidence=0.5):
        """khr_rv_check + khr_rv_detect_changes: RayVerificator::check and RayChangeDetector::detectChanges for all points
        without the stamp lists leaving the device.  forward: bool or per-point array.
        -> (closest_absent[m], furthest_persistent[m], flags[m]) (flags: bit 0 / bit 1 = exists, bit 7 = vote on the host)."""
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        m = pts.shape[0]
        t0 = np.ascontiguousarray(np.broadcast_to(np.asarray(earliest, np.uint64), (m,)))
        t1 = np.ascontiguousarray(np.broadcast_to(np.asarray(latest, np.uint64), (m,)))
        tp, ta = C.c_uint64(0), C.c_uint64(0)
        self._chk(self.lib.khr_rv_check(self.h, m, _ptr(pts), _ptr(t0), _ptr(t1), None, None, C.byref(tp), C.byref(ta)))
        ca, fp, fl = np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint64), np.zeros(max(m, 1), np.uint8)
        if m:
            if np.isscalar(forward) or isinstance(forward, (bool, np.bool_)):
                fwd, fall = None, (1 if forward else -1)
            else:
                fwd, fall = np.ascontiguousarray(np.asarray(forward).astype(np.uint8)), 0
            self._chk(self.lib.khr_rv_detect_changes(self.h, float(temporal_resolution), int(window_size), 1 if use_relative_confidence else 0,
                                                     float(absence_confidence), float(presence_confidence), _ptr(fwd) if fwd is not None else None,
                                                     fall, _ptr(ca), _ptr(fp), _ptr(fl)))
        return ca[:m], fp[:m], fl[:m]
