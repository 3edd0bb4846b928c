"""ctypes binding of the C ABI (include/spz_amd.h, spz_amd/lib/libspz_amd.so).

This is the same boundary a cgo / JNI / N-API binding would use: plain pointers and sizes.
PyTorch only supplies device memory and streams to it (``tensor.data_ptr()``,
``torch.cuda.current_stream().cuda_stream``).  There is no CPU fallback: if the shared
library is missing or no HIP device is usable, calls raise.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# SPZ_AMD_LIB: another build of the library (tools/tune.py variants under a profiler); default: the in-tree build
LIB_PATH = os.environ.get("SPZ_AMD_LIB") or os.path.join(HERE, "lib", "libspz_amd.so")

OK = 0
ERR_INVALID_ARG = -1
ERR_HEADER_NOT_FOUND = -2
ERR_VERSION = -3
ERR_TOO_MANY_POINTS = -4
ERR_SH_DEGREE = -5
ERR_SHORT_STREAM = -6
ERR_CAPACITY = -7
ERR_NO_DEVICE = -8
ERR_HIP = -9
ERR_UNSUPPORTED = -10
ERR_COMM = -11
ERR_VERIFY = -12

UNSPECIFIED, LDB, RDB, LUB, RUB, LDF, RDF, LUF, RUF = range(9)
NUM_SECTIONS = 6
SEC_POSITIONS, SEC_ALPHAS, SEC_COLORS, SEC_SCALES, SEC_ROTATIONS, SEC_SH = range(6)
REFERENCE_MAX_POINTS = 10_000_000

# Every symbol include/spz_amd.h declares (tests check the library exports all of them).
EXPORTS = (
    "spz_amd_abi_version", "spz_amd_status_string", "spz_amd_device_count", "spz_amd_last_hip_error",
    "spz_amd_release_device_memory",
    "spz_amd_stream_layout", "spz_amd_write_header", "spz_amd_peek_header", "spz_amd_peek_header_ex",
    "spz_amd_peek_header_device",
    "spz_amd_encode_device", "spz_amd_decode_device", "spz_amd_encode_shard_device",
    "spz_amd_decode_shard_device", "spz_amd_decode_gather_device", "spz_amd_decode_gather_host",
    "spz_amd_convert_coordinates_device",
    "spz_amd_encode_host",
    "spz_amd_decode_host", "spz_amd_decode_host_ex", "spz_amd_decode_host_from_device", "spz_amd_convert_coordinates_host", "spz_amd_get_tables",
    "spz_amd_ply_default_columns", "spz_amd_ply_rows_to_cloud_device", "spz_amd_cloud_to_ply_rows_device",
    "spz_amd_ply_rows_to_cloud_host", "spz_amd_cloud_to_ply_rows_host",
    "spz_amd_median_scale_sum_device", "spz_amd_median_scale_sum_host",
    "spz_amd_selftest_device",
    "spz_amd_encode_shard_sections_device", "spz_amd_shard_fragments",
    "spz_amd_rccl_available", "spz_amd_last_rccl_error", "spz_amd_rccl_unique_id", "spz_amd_rccl_comm_init",
    "spz_amd_rccl_comm_destroy", "spz_amd_gatherv_rccl", "spz_amd_scatterv_rccl",
    "spz_amd_ipc_alloc", "spz_amd_ipc_free", "spz_amd_ipc_open", "spz_amd_ipc_close",
    "spz_amd_zlib_parse_open", "spz_amd_zlib_parse_open_ex", "spz_amd_zlib_parse_fetch", "spz_amd_zlib_parse_close",
    "spz_amd_zlib_parse_append", "spz_amd_zlib_block_stats", "spz_amd_zlib_encode_blocks", "spz_amd_zlib_verify_member",
    "spz_amd_zlib_encode_group", "spz_amd_zlib_encode_finish", "spz_amd_zlib_parse_open_dev", "spz_amd_encode_host_keep", "spz_amd_kept_stream_release",
    "spz_amd_zlib_block_trees", "spz_amd_zlib_encode_planned", "spz_amd_zlib_encode_finish_ex",
    "spz_amd_inflate_open", "spz_amd_inflate_open_ex", "spz_amd_inflate_open_device", "spz_amd_inflate_equals_device", "spz_amd_inflate_crc_piece_bytes", "spz_amd_inflate_piece_crcs", "spz_amd_inflate_fetch",
    "spz_amd_inflate_device_data", "spz_amd_inflate_close", "spz_amd_stream_to_device", "spz_amd_inflate_last_decline",
    "spz_amd_cloud_buffers_alloc", "spz_amd_cloud_buffers_free",
    "spz_amd_zlib_session_open", "spz_amd_zlib_session_feed", "spz_amd_zlib_session_close", "spz_amd_zlib_parse_open_session",
    "spz_amd_encode_host_keep_session", "spz_amd_encode_host_keep_session_tail", "spz_amd_decode_gather_host_from_device",
    "spz_amd_filter_workspace_bytes", "spz_amd_select_device", "spz_amd_subset_device",
    "spz_amd_filter_open", "spz_amd_filter_fetch", "spz_amd_filter_device_data", "spz_amd_filter_close",
    "spz_amd_transform_params", "spz_amd_transform_cloud_device", "spz_amd_transform_packed_device",
    "spz_amd_transform_open", "spz_amd_transform_fetch", "spz_amd_transform_device_data", "spz_amd_transform_close",
    "spz_amd_transform_cloud_host",
    "spz_amd_merge_resolve", "spz_amd_merge_workspace_bytes", "spz_amd_merge_device", "spz_amd_merge_open",
    "spz_amd_merge_fetch", "spz_amd_merge_device_data", "spz_amd_merge_close",
    "spz_amd_sort_workspace_bytes", "spz_amd_morton_order_device", "spz_amd_argsort_f32_device",
    "spz_amd_chunk_bounds_device", "spz_amd_sort_open", "spz_amd_sort_fetch", "spz_amd_sort_device_data",
    "spz_amd_sort_close",
    "spz_amd_decimate_workspace_bytes", "spz_amd_decimate_level_counts_device", "spz_amd_decimate_device",
    "spz_amd_decimate_open", "spz_amd_decimate_fetch", "spz_amd_decimate_device_data", "spz_amd_decimate_close",
    "spz_amd_tile_workspace_bytes", "spz_amd_tile_content_workspace_bytes", "spz_amd_tile_tree_device",
    "spz_amd_tile_content_device", "spz_amd_tile_open", "spz_amd_tile_table", "spz_amd_tile_fetch",
    "spz_amd_tile_fetch_arena", "spz_amd_tile_device_data", "spz_amd_tile_close",
    "spz_amd_clean_workspace_bytes", "spz_amd_clean_radius_r2", "spz_amd_knn_scores_device",
    "spz_amd_radius_counts_device", "spz_amd_clean_open", "spz_amd_clean_fetch", "spz_amd_clean_device_data",
    "spz_amd_clean_close",
    "spz_amd_align_default_options", "spz_amd_align_check", "spz_amd_align_workspace_bytes",
    "spz_amd_align_prepare_device", "spz_amd_nearest_device", "spz_amd_align_step_device", "spz_amd_align_solve",
    "spz_amd_align_host",
    "spz_amd_plane_default_options", "spz_amd_plane_check", "spz_amd_plane_threshold", "spz_amd_plane_workspace_bytes",
    "spz_amd_plane_prepare_device", "spz_amd_plane_gather_device", "spz_amd_plane_hypotheses",
    "spz_amd_plane_score_device", "spz_amd_plane_moments_device", "spz_amd_plane_solve", "spz_amd_plane_mark_device",
    "spz_amd_plane_placement", "spz_amd_plane_sides_host", "spz_amd_plane_host",
    "spz_amd_render_check_params", "spz_amd_render_workspace_bytes", "spz_amd_render_prepare_packed_device",
    "spz_amd_render_prepare_cloud_device", "spz_amd_render_finish_device", "spz_amd_render_host",
    "spz_amd_render_cloud_host", "spz_amd_render_score_device", "spz_amd_prune_keep_count", "spz_amd_prune_open",
    "spz_amd_prune_fetch", "spz_amd_prune_device_data", "spz_amd_prune_close",
    "spz_amd_render_depth_device", "spz_amd_render_depth_host", "spz_amd_render_depth_cloud_host",
    "spz_amd_render_backward_workspace_bytes", "spz_amd_render_backward_device",
    "spz_amd_render_depth_backward_workspace_bytes", "spz_amd_render_depth_backward_device",
    "spz_amd_depth_loss_workspace_bytes", "spz_amd_depth_loss_device", "spz_amd_depth_default_options",
    "spz_amd_depth_check", "spz_amd_refine_images_depth_open", "spz_amd_refine_images_depth_host_open",
    "spz_amd_image_metrics_check", "spz_amd_image_metrics_workspace_bytes", "spz_amd_image_metrics_device",
    "spz_amd_image_metrics_host", "spz_amd_compare_host",
    "spz_amd_image_loss_workspace_bytes", "spz_amd_image_loss_device", "spz_amd_adam_scalars_of",
    "spz_amd_adam_step_device", "spz_amd_refine_default_options", "spz_amd_refine_check", "spz_amd_refine_open",
    "spz_amd_refine_fetch", "spz_amd_refine_device_data", "spz_amd_refine_close",
    "spz_amd_densify_default_options", "spz_amd_densify_check", "spz_amd_densify_thresholds",
    "spz_amd_densify_accumulate_device", "spz_amd_densify_plan_workspace_bytes", "spz_amd_densify_plan_device",
    "spz_amd_densify_plan_host", "spz_amd_densify_apply_device", "spz_amd_densify_reset_opacity_device",
    "spz_amd_refine_densify_open",
    "spz_amd_photo_loss_workspace_bytes", "spz_amd_photo_loss_device", "spz_amd_image_exposure_device",
    "spz_amd_photo_default_options", "spz_amd_photo_check", "spz_amd_refine_images_open",
    "spz_amd_refine_images_host_open",
    "spz_amd_render_records_backward_device", "spz_amd_render_view_backward_workspace_bytes",
    "spz_amd_render_view_backward_device",
    "spz_amd_locate_default_options", "spz_amd_locate_check", "spz_amd_locate_level_params",
    "spz_amd_locate_twist_gradient", "spz_amd_locate_pose_step", "spz_amd_image_halve_device", "spz_amd_locate_host",
    "spz_amd_locate_image_host", "spz_amd_locate_cloud_host",
    "spz_amd_tsdf_check", "spz_amd_tsdf_bytes", "spz_amd_tsdf_volume_from_box", "spz_amd_tsdf_integrate_device",
    "spz_amd_mesh_tet_table", "spz_amd_mesh_workspace_bytes", "spz_amd_mesh_count_device", "spz_amd_mesh_emit_device",
    "spz_amd_mesh_default_options", "spz_amd_mesh_check", "spz_amd_mesh_open", "spz_amd_mesh_fetch",
    "spz_amd_mesh_close",
    "spz_amd_seed_default_options", "spz_amd_seed_check", "spz_amd_seed_samples", "spz_amd_seed_workspace_bytes",
    "spz_amd_seed_view_device", "spz_amd_seed_open", "spz_amd_seed_fetch", "spz_amd_seed_device_data",
    "spz_amd_seed_close",
)

RCCL_UNIQUE_ID_BYTES = 128
IPC_HANDLE_BYTES = 64
ALL_SECTIONS = 0x3f
SMALL_SECTIONS = 0x1f      # positions, alphas, colors, scales, rotations (20 B/point for v3)
SH_SECTION = 0x20


class Header(C.Structure):
    _fields_ = [("version", C.c_uint32), ("num_points", C.c_uint32), ("sh_degree", C.c_uint8),
                ("fractional_bits", C.c_uint8), ("flags", C.c_uint8), ("reserved", C.c_uint8)]

    @property
    def antialiased(self):
        return bool(self.flags & 1)


class Layout(C.Structure):
    _fields_ = [("total_bytes", C.c_uint64), ("offset", C.c_uint64 * NUM_SECTIONS),
                ("bytes", C.c_uint64 * NUM_SECTIONS), ("bytes_per_point", C.c_uint32 * NUM_SECTIONS)]


class CloudPtrs(C.Structure):
    """spz_amd_cloud_in / spz_amd_cloud_out / spz_amd_cloud_grads (same layout: six pointers)."""
    _fields_ = [(k, C.c_void_p) for k in ("positions", "scales", "rotations", "alphas", "colors", "sh")]


class RenderParams(C.Structure):
    """spz_amd_render_params: one pinhole view (OpenCV axes; include/spz_amd.h "render")."""
    _fields_ = [("world_to_camera", C.c_float * 12), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float),
                ("cy", C.c_float), ("width", C.c_uint32), ("height", C.c_uint32), ("near_plane", C.c_float),
                ("background", C.c_float * 3), ("max_sh_degree", C.c_int32), ("coord", C.c_int32)]


RENDER_RECORD_BYTES = 48
PRUNE_MAX_VIEWS = 1024
PRUNE_SCORE_SUM, PRUNE_SCORE_MAX = 0, 1
PRUNE_KEEP_COUNT, PRUNE_KEEP_FRACTION, PRUNE_MIN_SCORE = 0, 1, 2
COMPARE_MAX_VIEWS = 1024


class AlignCloud(C.Structure):
    """spz_amd_align_cloud: one cloud of an alignment (device stream, its size and header)."""
    _fields_ = [("d_stream", C.c_void_p), ("size", C.c_size_t), ("hdr", Header)]


class AlignOptions(C.Structure):
    """spz_amd_align_options (include/spz_amd.h "align"); spz_amd_align_default_options fills the defaults."""
    _fields_ = [("rotation", C.c_double * 4), ("translation", C.c_double * 3), ("scale", C.c_double),
                ("coord", C.c_int32), ("estimate_scale", C.c_int32), ("overlap", C.c_double),
                ("max_distance", C.c_double), ("has_max_distance", C.c_int32), ("stride", C.c_uint32),
                ("max_iterations", C.c_uint32), ("init_centroids", C.c_int32), ("relative_fitness", C.c_double),
                ("relative_rmse", C.c_double)]


class AlignMoments(C.Structure):
    """spz_amd_align_moments: the sums of one step over its inliers (sum d2 = sum_d2_hi 2^64 + sum_d2_lo)."""
    _fields_ = [("count", C.c_uint64), ("taking_part", C.c_uint64), ("candidates", C.c_uint64),
                ("sum_d2_lo", C.c_uint64), ("sum_d2_hi", C.c_uint64), ("sum_a", C.c_double * 3),
                ("sum_b", C.c_double * 3), ("sum_ab", C.c_double * 9), ("sum_aa", C.c_double), ("sum_bb", C.c_double)]


class Plane(C.Structure):
    """spz_amd_plane: d = a X + b Y + c Z - e on the stored integers (include/spz_amd.h "plane")."""
    _fields_ = [("a", C.c_int32), ("b", C.c_int32), ("c", C.c_int32), ("reserved", C.c_int32), ("e", C.c_int64)]


class PlaneOptions(C.Structure):
    """spz_amd_plane_options; spz_amd_plane_default_options fills the defaults (threshold has none)."""
    _fields_ = [("threshold", C.c_double), ("hypotheses", C.c_uint32), ("refine", C.c_uint32),
                ("max_planes", C.c_uint32), ("stride", C.c_uint32), ("seed", C.c_uint64), ("min_inliers", C.c_uint64),
                ("has_axis", C.c_int32), ("axis", C.c_double * 3), ("max_tilt", C.c_double),
                ("has_up_hint", C.c_int32), ("up_hint", C.c_double * 3), ("coord", C.c_int32),
                ("no_translate", C.c_int32)]


class PlaneMoments(C.Structure):
    """spz_amd_plane_moments: the exact sums of one plane over its inliers (sum_pp = hi 2^64 + lo, two's complement)."""
    _fields_ = [("count", C.c_uint64), ("sum_abs", C.c_uint64), ("above", C.c_uint64), ("below", C.c_uint64),
                ("points", C.c_uint64), ("sum_p", C.c_int64 * 3), ("sum_pp_lo", C.c_uint64 * 6),
                ("sum_pp_hi", C.c_int64 * 6)]


class PlaneResult(C.Structure):
    """spz_amd_plane_result: one plane of a run with its levelling placement."""
    _fields_ = [("plane", Plane), ("inliers", C.c_uint64), ("sum_abs", C.c_uint64), ("points", C.c_uint64),
                ("above", C.c_uint64), ("below", C.c_uint64), ("best_hypothesis", C.c_uint32),
                ("refinements", C.c_uint32), ("fitness", C.c_double), ("mean_distance", C.c_double),
                ("normal", C.c_double * 3), ("offset", C.c_double), ("rotation", C.c_double * 4),
                ("translation", C.c_double * 3), ("scale", C.c_double)]


class AlignHistory(C.Structure):
    _fields_ = [("fitness", C.c_double), ("inlier_rmse", C.c_double), ("inliers", C.c_uint64)]


class AlignResult(C.Structure):
    """spz_amd_align_result: the map used by the last step (rotation, translation, scale in coord; map in the stored
    frame) with that step's fitness, rmse and inlier count."""
    _fields_ = [("rotation", C.c_double * 4), ("translation", C.c_double * 3), ("scale", C.c_double),
                ("map", C.c_double * 12), ("fitness", C.c_double), ("inlier_rmse", C.c_double),
                ("inliers", C.c_uint64), ("iterations", C.c_uint32), ("converged", C.c_int32),
                ("degenerate", C.c_int32)]


NO_NEIGHBOUR = 0xFFFFFFFF      # spz_amd_nearest_device's index of a point without one
NO_LIMIT_R2 = (1 << 64) - 1    # its r2 for "no distance limit"


class ImageMetrics(C.Structure):
    """spz_amd_image_metrics: the five results of one image pair (include/spz_amd.h "image metrics")."""
    _fields_ = [("mse", C.c_double), ("psnr", C.c_double), ("ssim", C.c_double), ("l1", C.c_double),
                ("max_abs", C.c_double)]


REFINE_MAX_VIEWS = 1024
TRAIN_ARRAYS = ("positions", "scales", "rotations", "alphas", "colors", "sh")   # bit k of a train_mask
TRAIN_ALL = 63
DEPTH_L1, DEPTH_INVERSE_L1 = 0, 1  # the depth loss's kinds


class AdamScalars(C.Structure):
    """spz_amd_adam_scalars: the f32 scalars of one Adam step (include/spz_amd.h "adam step")."""
    _fields_ = [("beta1", C.c_float), ("c1", C.c_float), ("beta2", C.c_float), ("c2", C.c_float), ("eps", C.c_float),
                ("r", C.c_float), ("s", C.c_float * 6)]


class RefineOptions(C.Structure):
    """spz_amd_refine_options (include/spz_amd.h "refine")."""
    _fields_ = [("iterations", C.c_int32), ("train_mask", C.c_uint32), ("lambda_dssim", C.c_double),
                ("lr", C.c_double * 6), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


class PhotoOptions(C.Structure):
    """spz_amd_photo_options (include/spz_amd.h "refine images")."""
    _fields_ = [("fit_exposure", C.c_int32), ("reserved", C.c_int32), ("lr_exposure", C.c_double)]


class DepthOptions(C.Structure):
    """spz_amd_depth_options (include/spz_amd.h "refine images with depth")."""
    _fields_ = [("weight", C.c_double), ("min_alpha", C.c_float), ("kind", C.c_int32)]


EXPOSURE_IDENTITY = (1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)   # row-major [M | o]

LOCATE_MAX_LEVELS = 8


class LocateOptions(C.Structure):
    """spz_amd_locate_options (include/spz_amd.h "locate")."""
    _fields_ = [("iterations", C.c_int32), ("levels", C.c_int32), ("lambda_dssim", C.c_double),
                ("lr_rotation", C.c_double), ("lr_translation", C.c_double), ("lr_final_factor", C.c_double),
                ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double)]


MESH_MAX_VIEWS = 1024
MESH_DEPTH_MEDIAN, MESH_DEPTH_EXPECTED = 0, 1
MESH_DEPTH_KINDS = {"median": MESH_DEPTH_MEDIAN, "expected": MESH_DEPTH_EXPECTED}


class TsdfVolume(C.Structure):
    """spz_amd_tsdf_volume: a lattice of dims sample points at lo + (i, j, k) voxel_size (include/spz_amd.h "mesh")."""
    _fields_ = [("lo", C.c_float * 3), ("voxel_size", C.c_float), ("dims", C.c_uint32 * 3), ("truncation", C.c_float)]


class MeshOptions(C.Structure):
    """spz_amd_mesh_options (include/spz_amd.h "mesh"); spz_amd_mesh_default_options fills the defaults."""
    _fields_ = [("box", C.c_double * 6), ("voxel_size", C.c_double), ("truncation", C.c_double),
                ("has_box", C.c_int32), ("resolution", C.c_int32), ("depth_kind", C.c_int32),
                ("min_alpha", C.c_float), ("min_weight", C.c_float), ("reserved", C.c_int32)]


SEED_MAX_VIEWS = 1024


class SeedOptions(C.Structure):
    """spz_amd_seed_options (include/spz_amd.h "seed"); spz_amd_seed_default_options fills the defaults.  alpha is the
    pre-sigmoid opacity."""
    _fields_ = [("stride", C.c_uint32), ("scale_factor", C.c_float), ("alpha", C.c_float), ("cover_alpha", C.c_float),
                ("cover_tolerance", C.c_float), ("cover", C.c_int32), ("sh_degree", C.c_int32), ("reserved", C.c_int32)]


class DensifyOptions(C.Structure):
    """spz_amd_densify_options (include/spz_amd.h "densify"); interval 0 = off."""
    _fields_ = [("interval", C.c_int32), ("from_iter", C.c_int32), ("until_iter", C.c_int32),
                ("opacity_reset_interval", C.c_int32), ("grad_threshold", C.c_double), ("percent_dense", C.c_double),
                ("extent", C.c_double), ("min_opacity", C.c_double), ("max_scale", C.c_double),
                ("max_points", C.c_uint64), ("seed", C.c_uint64)]


class DensifyLimits(C.Structure):
    """spz_amd_densify_limits: the f32 thresholds the plan kernel compares against, and the extent they came from."""
    _fields_ = [("grad_threshold", C.c_float), ("log_dense", C.c_float), ("alpha_min", C.c_float),
                ("log_max_scale", C.c_float), ("use_max_scale", C.c_int32), ("reserved", C.c_int32),
                ("extent", C.c_double)]


class DensifyRound(C.Structure):
    """spz_amd_densify_round: what one round of refine's densify did."""
    _fields_ = [("iteration", C.c_int32), ("reserved", C.c_int32), ("cloned", C.c_uint64), ("split", C.c_uint64),
                ("culled", C.c_uint64), ("refused", C.c_uint64), ("num_points", C.c_uint64)]


DENSIFY_KEEP, DENSIFY_CLONE, DENSIFY_SPLIT, DENSIFY_CULL = 0, 1, 2, 3   # d_action's values
DENSIFY_FIELDS = ("interval", "from_iter", "until_iter", "opacity_reset_interval", "grad_threshold", "percent_dense",
                  "extent", "min_opacity", "max_scale", "max_points", "seed")


class TileInfo(C.Structure):
    """spz_amd_tile_info: one row of a tile table (include/spz_amd.h "tile"); 104 bytes."""
    _fields_ = [("id", C.c_uint32), ("parent", C.c_int32), ("first_child", C.c_int32), ("child_count", C.c_uint32),
                ("level", C.c_int32), ("cell", C.c_uint32 * 3), ("range_begin", C.c_uint32), ("range_end", C.c_uint32),
                ("content_level", C.c_int32), ("num_points", C.c_uint32), ("content_begin", C.c_uint32),
                ("reserved", C.c_uint32), ("offset", C.c_uint64), ("bytes", C.c_uint64), ("box_min", C.c_float * 3),
                ("box_max", C.c_float * 3), ("max_radius", C.c_float), ("geometric_error", C.c_float)]


class TileSummary(C.Structure):
    """spz_amd_tile_summary: what spz_amd_tile_tree_device leaves beside the table."""
    _fields_ = [("num_tiles", C.c_uint64), ("arena_bytes", C.c_uint64), ("ok", C.c_uint32), ("root_level", C.c_uint32),
                ("cells", C.c_uint64 * 25)]


TILE_DEFAULT_MAX_TILES = 65536


class CloudBuffers(C.Structure):
    """spz_amd_cloud_buffers: device buffers made (and placed) by spz_amd_cloud_buffers_alloc."""
    _fields_ = [("cloud", CloudPtrs), ("stream", C.c_void_p), ("stream_capacity", C.c_size_t), ("owner", C.c_void_p),
                ("candidates", C.c_int32), ("probe_ms_first", C.c_float), ("probe_ms_chosen", C.c_float),
                ("probe_ms_worst", C.c_float)]


class PlyColumns(C.Structure):
    """spz_amd_ply_columns: column map of a .ply vertex row."""
    _fields_ = [("stride", C.c_int32), ("sh_dim", C.c_int32), ("position", C.c_int32 * 3), ("scale", C.c_int32 * 3),
                ("rotation", C.c_int32 * 4), ("alpha", C.c_int32), ("color", C.c_int32 * 3), ("sh", C.c_int32 * 45)]


class Fragments(C.Structure):
    """spz_amd_fragments: the six byte ranges of a point-range shard."""
    _fields_ = [("global_offset", C.c_uint64 * NUM_SECTIONS), ("local_offset", C.c_uint64 * NUM_SECTIONS),
                ("bytes", C.c_uint64 * NUM_SECTIONS)]


class Selection(C.Structure):
    """spz_amd_selection: the predicates of spz_amd_select_device (box inclusive, alpha on the decoded logit)."""
    _fields_ = [("to_coord", C.c_int32), ("use_box", C.c_int32), ("box_lo", C.c_float * 3), ("box_hi", C.c_float * 3),
                ("use_min_alpha", C.c_int32), ("min_alpha", C.c_float)]


class Transform(C.Structure):
    """spz_amd_transform: the f32 parameter block of spz_amd_transform_params (M = s*R row-major, t, ln_s, unit q_R,
    the sh band matrices D_l[k][m] row-major, and which steps run)."""
    _fields_ = [("m", C.c_float * 9), ("t", C.c_float * 3), ("ln_s", C.c_float), ("q", C.c_float * 4),
                ("d1", C.c_float * 9), ("d2", C.c_float * 25), ("d3", C.c_float * 49),
                ("apply_positions", C.c_int32), ("apply_scales", C.c_int32), ("apply_rotation", C.c_int32)]


MERGE_MAX_INPUTS = 1024   # SPZ_AMD_MERGE_MAX_INPUTS


class MergeInput(C.Structure):
    """spz_amd_merge_input: one input of a merge (device stream, its size and header, NULL or a placement block)."""
    _fields_ = [("d_stream", C.c_void_p), ("size", C.c_size_t), ("hdr", Header), ("xf", C.POINTER(Transform))]


class SpzAmdError(RuntimeError):
    def __init__(self, status, where):
        self.status = status
        super().__init__(f"{where}: {status_string(status)} (status {status})")


MEDIAN_WORKSPACE_BYTES = 8192   # SPZ_AMD_MEDIAN_WORKSPACE_BYTES

_lib = None


def load_library():
    """Load libspz_amd.so.  torch is imported first (when available) so that the HIP runtime
    torch ships is the one both share (same SONAME libamdhip64.so.7)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} not found: build it with `make` (or __graft_entry__.build()); "
                           "spz_amd has no CPU fallback")
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    _lib = bind(C.CDLL(LIB_PATH))
    return _lib


def bind(L):
    """Declare the C ABI's argument / result types on a loaded library handle."""
    vp, u64, i32, sz = C.c_void_p, C.c_uint64, C.c_int, C.c_size_t
    L.spz_amd_abi_version.restype = i32
    L.spz_amd_status_string.restype = C.c_char_p
    L.spz_amd_status_string.argtypes = [i32]
    L.spz_amd_device_count.restype = i32
    L.spz_amd_last_hip_error.restype = i32
    L.spz_amd_release_device_memory.restype = i32
    L.spz_amd_stream_layout.restype = i32
    L.spz_amd_stream_layout.argtypes = [u64, i32, i32, C.POINTER(Layout)]
    L.spz_amd_write_header.restype = i32
    L.spz_amd_write_header.argtypes = [C.POINTER(Header), vp]
    L.spz_amd_peek_header.restype = i32
    L.spz_amd_peek_header.argtypes = [vp, sz, C.POINTER(Header)]
    L.spz_amd_peek_header_ex.restype = i32
    L.spz_amd_peek_header_ex.argtypes = [vp, sz, u64, C.POINTER(Header)]
    L.spz_amd_peek_header_device.restype = i32
    L.spz_amd_peek_header_device.argtypes = [vp, sz, u64, C.POINTER(Header), vp]
    L.spz_amd_encode_device.restype = i32
    L.spz_amd_encode_device.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, i32, i32, vp, sz, vp]
    L.spz_amd_decode_device.restype = i32
    L.spz_amd_decode_device.argtypes = [vp, sz, C.POINTER(Header), i32, C.POINTER(CloudPtrs), vp]
    L.spz_amd_encode_shard_device.restype = i32
    L.spz_amd_encode_shard_device.argtypes = [C.POINTER(CloudPtrs), u64, u64, u64, i32, i32, i32, i32, i32, vp, sz, vp]
    L.spz_amd_decode_shard_device.restype = i32
    L.spz_amd_decode_shard_device.argtypes = [vp, sz, C.POINTER(Header), u64, u64, i32, C.POINTER(CloudPtrs), vp]
    L.spz_amd_decode_gather_device.restype = i32
    L.spz_amd_decode_gather_device.argtypes = [vp, sz, C.POINTER(Header), vp, u64, i32, C.POINTER(CloudPtrs), vp]
    L.spz_amd_median_scale_sum_device.restype = i32
    L.spz_amd_median_scale_sum_device.argtypes = [vp, u64, vp, vp, vp]
    L.spz_amd_median_scale_sum_host.restype = i32
    L.spz_amd_median_scale_sum_host.argtypes = [vp, u64, vp, i32]
    L.spz_amd_cloud_buffers_alloc.restype = i32
    L.spz_amd_cloud_buffers_alloc.argtypes = [u64, i32, i32, vp, i32, i32, vp, C.POINTER(CloudBuffers)]
    L.spz_amd_cloud_buffers_free.restype = i32
    L.spz_amd_cloud_buffers_free.argtypes = [C.POINTER(CloudBuffers)]
    L.spz_amd_decode_gather_host.restype = i32
    L.spz_amd_decode_gather_host.argtypes = [vp, sz, u64, vp, u64, i32, C.POINTER(CloudPtrs), i32]
    L.spz_amd_convert_coordinates_device.restype = i32
    L.spz_amd_convert_coordinates_device.argtypes = [vp, vp, vp, u64, i32, i32, i32, vp]
    L.spz_amd_encode_host.restype = i32
    L.spz_amd_encode_host.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, i32, i32, vp, sz, i32]
    L.spz_amd_decode_host.restype = i32
    L.spz_amd_decode_host.argtypes = [vp, sz, i32, C.POINTER(CloudPtrs), i32]
    L.spz_amd_decode_host_ex.restype = i32
    L.spz_amd_decode_host_ex.argtypes = [vp, sz, u64, i32, C.POINTER(CloudPtrs), i32]
    L.spz_amd_convert_coordinates_host.restype = i32
    L.spz_amd_convert_coordinates_host.argtypes = [vp, vp, vp, u64, i32, i32, i32, i32]
    L.spz_amd_get_tables.restype = i32
    L.spz_amd_get_tables.argtypes = [vp, vp, vp]
    L.spz_amd_ply_default_columns.restype = i32
    L.spz_amd_ply_default_columns.argtypes = [i32, C.POINTER(PlyColumns)]
    L.spz_amd_ply_rows_to_cloud_device.restype = i32
    L.spz_amd_ply_rows_to_cloud_device.argtypes = [vp, u64, C.POINTER(PlyColumns), i32, C.POINTER(CloudPtrs), vp]
    L.spz_amd_cloud_to_ply_rows_device.restype = i32
    L.spz_amd_cloud_to_ply_rows_device.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, vp, vp]
    L.spz_amd_ply_rows_to_cloud_host.restype = i32
    L.spz_amd_ply_rows_to_cloud_host.argtypes = [vp, u64, C.POINTER(PlyColumns), i32, C.POINTER(CloudPtrs), i32]
    L.spz_amd_cloud_to_ply_rows_host.restype = i32
    L.spz_amd_cloud_to_ply_rows_host.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, vp, i32]
    u32 = C.c_uint
    L.spz_amd_encode_shard_sections_device.restype = i32
    L.spz_amd_encode_shard_sections_device.argtypes = [C.POINTER(CloudPtrs), u64, u64, u64, i32, i32, i32, i32, i32, u32, vp, sz, vp]
    L.spz_amd_shard_fragments.restype = i32
    L.spz_amd_shard_fragments.argtypes = [u64, u64, u64, i32, i32, C.POINTER(Fragments)]
    L.spz_amd_rccl_available.restype = i32
    L.spz_amd_last_rccl_error.restype = i32
    L.spz_amd_rccl_unique_id.restype = i32
    L.spz_amd_rccl_unique_id.argtypes = [vp]
    L.spz_amd_rccl_comm_init.restype = i32
    L.spz_amd_rccl_comm_init.argtypes = [vp, i32, i32, C.POINTER(vp)]
    L.spz_amd_rccl_comm_destroy.restype = i32
    L.spz_amd_rccl_comm_destroy.argtypes = [vp]
    L.spz_amd_gatherv_rccl.restype = i32
    L.spz_amd_gatherv_rccl.argtypes = [vp, i32, i32, i32, C.POINTER(u64), C.POINTER(u64), i32, i32, vp, vp, u32, vp]
    L.spz_amd_scatterv_rccl.restype = i32
    L.spz_amd_scatterv_rccl.argtypes = [vp, i32, i32, i32, C.POINTER(u64), C.POINTER(u64), i32, i32, vp, vp, u32, vp]
    L.spz_amd_ipc_alloc.restype = i32
    L.spz_amd_ipc_alloc.argtypes = [sz, C.POINTER(vp), vp]
    L.spz_amd_ipc_free.restype = i32
    L.spz_amd_ipc_free.argtypes = [vp]
    L.spz_amd_ipc_open.restype = i32
    L.spz_amd_ipc_open.argtypes = [vp, C.POINTER(vp)]
    L.spz_amd_ipc_close.restype = i32
    L.spz_amd_ipc_close.argtypes = [vp]
    L.spz_amd_selftest_device.restype = i32
    L.spz_amd_selftest_device.argtypes = [i32, u64, u64, C.POINTER(u64 * 3), vp]
    L.spz_amd_zlib_parse_open.restype = i32
    L.spz_amd_zlib_parse_open.argtypes = [vp, u64, u64, vp, u32, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u32)]
    L.spz_amd_zlib_parse_open_ex.restype = i32
    L.spz_amd_zlib_parse_open_ex.argtypes = [vp, u64, u64, vp, u32, i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u32), vp, vp]
    L.spz_amd_zlib_parse_fetch.restype = i32
    L.spz_amd_zlib_parse_fetch.argtypes = [vp, vp, vp]
    L.spz_amd_zlib_parse_close.restype = None
    L.spz_amd_zlib_parse_close.argtypes = [vp]
    L.spz_amd_zlib_parse_append.restype = i32
    L.spz_amd_zlib_parse_append.argtypes = [vp, vp, vp, u64]
    L.spz_amd_zlib_block_stats.restype = i32
    L.spz_amd_zlib_block_stats.argtypes = [vp, vp, u32, u32, vp, vp, vp, vp]
    L.spz_amd_decode_host_from_device.restype = i32
    L.spz_amd_decode_host_from_device.argtypes = [vp, sz, vp, i32, vp, i32]
    L.spz_amd_inflate_open.restype = i32
    L.spz_amd_inflate_open.argtypes = [vp, u64, i32, C.POINTER(vp), C.POINTER(u64)]
    L.spz_amd_inflate_crc_piece_bytes.restype = u32
    L.spz_amd_inflate_crc_piece_bytes.argtypes = []
    L.spz_amd_inflate_piece_crcs.restype = i32
    L.spz_amd_inflate_piece_crcs.argtypes = [vp, vp, u32, C.POINTER(u32)]
    L.spz_amd_inflate_fetch.restype = i32
    L.spz_amd_inflate_fetch.argtypes = [vp, vp]
    L.spz_amd_inflate_device_data.restype = vp
    L.spz_amd_inflate_device_data.argtypes = [vp]
    L.spz_amd_inflate_close.restype = None
    L.spz_amd_inflate_close.argtypes = [vp]
    L.spz_amd_zlib_encode_group.restype = i32
    L.spz_amd_zlib_encode_group.argtypes = [vp, vp, u32, u32, u32, u32, vp, vp, vp, u64, u64]
    L.spz_amd_zlib_encode_finish.restype = i32
    L.spz_amd_zlib_encode_finish.argtypes = [vp, u32, u64, vp, vp]
    L.spz_amd_zlib_block_trees.restype = i32
    L.spz_amd_zlib_block_trees.argtypes = [vp, u32, vp]
    L.spz_amd_zlib_encode_planned.restype = i32
    L.spz_amd_zlib_encode_planned.argtypes = [vp, vp, u32, u32, vp, u64]
    L.spz_amd_zlib_encode_finish_ex.restype = i32
    L.spz_amd_zlib_encode_finish_ex.argtypes = [vp, u32, u64, vp, vp, vp]
    L.spz_amd_filter_workspace_bytes.restype = u64
    L.spz_amd_filter_workspace_bytes.argtypes = [u64]
    L.spz_amd_select_device.restype = i32
    L.spz_amd_select_device.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(Selection), vp, vp, vp, C.POINTER(u64), vp]
    L.spz_amd_subset_device.restype = i32
    L.spz_amd_subset_device.argtypes = [vp, sz, C.POINTER(Header), vp, u64, i32, vp, sz, vp]
    L.spz_amd_filter_open.restype = i32
    L.spz_amd_filter_open.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(Selection), vp, i32, vp, u64, i32, i32,
                                      C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), vp]
    L.spz_amd_filter_fetch.restype = i32
    L.spz_amd_filter_fetch.argtypes = [vp, vp]
    L.spz_amd_filter_device_data.restype = vp
    L.spz_amd_filter_device_data.argtypes = [vp]
    L.spz_amd_filter_close.restype = None
    L.spz_amd_filter_close.argtypes = [vp]
    d3 = C.POINTER(C.c_double)
    L.spz_amd_transform_params.restype = i32
    L.spz_amd_transform_params.argtypes = [d3, d3, C.c_double, i32, C.POINTER(Transform)]
    L.spz_amd_transform_cloud_device.restype = i32
    L.spz_amd_transform_cloud_device.argtypes = [vp, vp, vp, vp, u64, i32, C.POINTER(Transform), vp]
    L.spz_amd_transform_packed_device.restype = i32
    L.spz_amd_transform_packed_device.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(Transform), i32, vp, sz, vp, vp]
    L.spz_amd_transform_open.restype = i32
    L.spz_amd_transform_open.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(Transform), i32, i32, C.POINTER(vp),
                                         C.POINTER(u64), C.POINTER(u64), vp]
    L.spz_amd_transform_fetch.restype = i32
    L.spz_amd_transform_fetch.argtypes = [vp, vp]
    L.spz_amd_transform_device_data.restype = vp
    L.spz_amd_transform_device_data.argtypes = [vp]
    L.spz_amd_transform_close.restype = None
    L.spz_amd_transform_close.argtypes = [vp]
    L.spz_amd_transform_cloud_host.restype = i32
    L.spz_amd_transform_cloud_host.argtypes = [vp, vp, vp, vp, u64, i32, C.POINTER(Transform), i32]
    L.spz_amd_merge_resolve.restype = i32
    L.spz_amd_merge_resolve.argtypes = [C.POINTER(Header), u64, i32, i32, i32, C.POINTER(Header), C.POINTER(u64)]
    L.spz_amd_merge_workspace_bytes.restype = u64
    L.spz_amd_merge_workspace_bytes.argtypes = [u64]
    L.spz_amd_merge_device.restype = i32
    L.spz_amd_merge_device.argtypes = [C.POINTER(MergeInput), u64, C.POINTER(Header), vp, sz, vp, vp, vp]
    L.spz_amd_merge_open.restype = i32
    L.spz_amd_merge_open.argtypes = [C.POINTER(MergeInput), u64, i32, i32, i32, i32, C.POINTER(vp), C.POINTER(Header),
                                     C.POINTER(u64), C.POINTER(u64), vp]
    L.spz_amd_merge_fetch.restype = i32
    L.spz_amd_merge_fetch.argtypes = [vp, vp]
    L.spz_amd_merge_device_data.restype = vp
    L.spz_amd_merge_device_data.argtypes = [vp]
    L.spz_amd_merge_close.restype = None
    L.spz_amd_merge_close.argtypes = [vp]
    L.spz_amd_sort_workspace_bytes.restype = u64
    L.spz_amd_sort_workspace_bytes.argtypes = [u64]
    L.spz_amd_morton_order_device.restype = i32
    L.spz_amd_morton_order_device.argtypes = [vp, sz, C.POINTER(Header), i32, vp, vp, vp]
    L.spz_amd_argsort_f32_device.restype = i32
    L.spz_amd_argsort_f32_device.argtypes = [vp, u64, i32, vp, vp, vp]
    L.spz_amd_chunk_bounds_device.restype = i32
    L.spz_amd_chunk_bounds_device.argtypes = [vp, sz, C.POINTER(Header), u32, vp, vp]
    L.spz_amd_sort_open.restype = i32
    L.spz_amd_sort_open.argtypes = [vp, sz, C.POINTER(Header), vp, i32, i32, C.POINTER(vp), C.POINTER(u64), vp, vp]
    L.spz_amd_sort_fetch.restype = i32
    L.spz_amd_sort_fetch.argtypes = [vp, vp]
    L.spz_amd_sort_device_data.restype = vp
    L.spz_amd_sort_device_data.argtypes = [vp]
    L.spz_amd_sort_close.restype = None
    L.spz_amd_sort_close.argtypes = [vp]
    L.spz_amd_decimate_workspace_bytes.restype = u64
    L.spz_amd_decimate_workspace_bytes.argtypes = [u64, i32]
    L.spz_amd_decimate_level_counts_device.restype = i32
    L.spz_amd_decimate_level_counts_device.argtypes = [vp, sz, C.POINTER(Header), vp, vp, vp]
    L.spz_amd_decimate_device.restype = i32
    L.spz_amd_decimate_device.argtypes = [vp, sz, C.POINTER(Header), i32, vp, sz, vp, vp, vp]
    L.spz_amd_decimate_open.restype = i32
    L.spz_amd_decimate_open.argtypes = [vp, sz, C.POINTER(Header), i32, u64, i32, C.POINTER(vp), C.POINTER(u64),
                                        C.POINTER(i32), C.POINTER(Header), vp, vp]
    L.spz_amd_decimate_fetch.restype = i32
    L.spz_amd_decimate_fetch.argtypes = [vp, vp]
    L.spz_amd_decimate_device_data.restype = vp
    L.spz_amd_decimate_device_data.argtypes = [vp]
    L.spz_amd_decimate_close.restype = None
    L.spz_amd_decimate_close.argtypes = [vp]
    L.spz_amd_tile_workspace_bytes.restype = u64
    L.spz_amd_tile_workspace_bytes.argtypes = [u64, i32, u64]
    L.spz_amd_tile_content_workspace_bytes.restype = u64
    L.spz_amd_tile_content_workspace_bytes.argtypes = [u64]
    L.spz_amd_tile_tree_device.restype = i32
    L.spz_amd_tile_tree_device.argtypes = [vp, sz, C.POINTER(Header), C.c_uint32, C.c_uint32, vp, vp, vp, vp]
    L.spz_amd_tile_content_device.restype = i32
    L.spz_amd_tile_content_device.argtypes = [vp, C.c_uint32, i32, vp, sz, vp, u64, vp, vp]
    L.spz_amd_tile_open.restype = i32
    L.spz_amd_tile_open.argtypes = [vp, sz, C.POINTER(Header), C.c_uint32, C.c_uint32, i32, C.POINTER(vp),
                                    C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_float)]
    L.spz_amd_tile_table.restype = i32
    L.spz_amd_tile_table.argtypes = [vp, vp]
    L.spz_amd_tile_fetch.restype = i32
    L.spz_amd_tile_fetch.argtypes = [vp, C.c_uint32, vp]
    L.spz_amd_tile_fetch_arena.restype = i32
    L.spz_amd_tile_fetch_arena.argtypes = [vp, vp]
    L.spz_amd_tile_device_data.restype = vp
    L.spz_amd_tile_device_data.argtypes = [vp, C.c_uint32]
    L.spz_amd_tile_close.restype = None
    L.spz_amd_tile_close.argtypes = [vp]
    L.spz_amd_clean_workspace_bytes.restype = u64
    L.spz_amd_clean_workspace_bytes.argtypes = [u64]
    L.spz_amd_clean_radius_r2.restype = i32
    L.spz_amd_clean_radius_r2.argtypes = [C.c_double, i32, C.POINTER(u64)]
    L.spz_amd_knn_scores_device.restype = i32
    L.spz_amd_knn_scores_device.argtypes = [vp, sz, C.POINTER(Header), i32, vp, vp, vp, vp]
    L.spz_amd_radius_counts_device.restype = i32
    L.spz_amd_radius_counts_device.argtypes = [vp, sz, C.POINTER(Header), u64, u32, vp, vp, vp]
    L.spz_amd_clean_open.restype = i32
    L.spz_amd_clean_open.argtypes = [vp, sz, C.POINTER(Header), i32, C.c_double, C.c_double, u32, i32, C.POINTER(vp),
                                     C.POINTER(u64), C.POINTER(u64), C.POINTER(C.c_double), vp, vp, vp]
    L.spz_amd_clean_fetch.restype = i32
    L.spz_amd_clean_fetch.argtypes = [vp, vp]
    L.spz_amd_clean_device_data.restype = vp
    L.spz_amd_clean_device_data.argtypes = [vp]
    L.spz_amd_clean_close.restype = None
    L.spz_amd_clean_close.argtypes = [vp]
    ac = C.POINTER(AlignCloud)
    L.spz_amd_align_default_options.restype = i32
    L.spz_amd_align_default_options.argtypes = [C.POINTER(AlignOptions)]
    L.spz_amd_align_check.restype = i32
    L.spz_amd_align_check.argtypes = [C.POINTER(AlignOptions)]
    L.spz_amd_align_workspace_bytes.restype = u64
    L.spz_amd_align_workspace_bytes.argtypes = [u64, u64]
    L.spz_amd_align_prepare_device.restype = i32
    L.spz_amd_align_prepare_device.argtypes = [ac, ac, vp, vp]
    L.spz_amd_nearest_device.restype = i32
    L.spz_amd_nearest_device.argtypes = [ac, ac, u32, C.POINTER(C.c_double), u64, vp, vp, vp, vp]
    L.spz_amd_align_step_device.restype = i32
    L.spz_amd_align_step_device.argtypes = [ac, ac, u32, C.POINTER(C.c_double), u64, C.c_double, vp, vp, vp, vp, vp, vp]
    L.spz_amd_align_solve.restype = i32
    L.spz_amd_align_solve.argtypes = [C.POINTER(AlignMoments), i32, C.c_double, C.POINTER(C.c_double),
                                      C.POINTER(C.c_double), C.POINTER(i32)]
    L.spz_amd_align_host.restype = i32
    L.spz_amd_align_host.argtypes = [ac, ac, C.POINTER(AlignOptions), i32, C.POINTER(AlignResult),
                                     C.POINTER(AlignHistory), u32, C.POINTER(C.c_float)]
    pp, dp = C.POINTER(Plane), C.POINTER(C.c_double)
    L.spz_amd_plane_default_options.restype = i32
    L.spz_amd_plane_default_options.argtypes = [C.POINTER(PlaneOptions)]
    L.spz_amd_plane_check.restype = i32
    L.spz_amd_plane_check.argtypes = [C.POINTER(PlaneOptions)]
    L.spz_amd_plane_threshold.restype = i32
    L.spz_amd_plane_threshold.argtypes = [C.c_double, i32, C.POINTER(u64)]
    L.spz_amd_plane_workspace_bytes.restype = u64
    L.spz_amd_plane_workspace_bytes.argtypes = [u64]
    L.spz_amd_plane_prepare_device.restype = i32
    L.spz_amd_plane_prepare_device.argtypes = [vp, C.c_size_t, C.POINTER(Header), u32, vp, vp, C.POINTER(u64), vp]
    L.spz_amd_plane_gather_device.restype = i32
    L.spz_amd_plane_gather_device.argtypes = [vp, u64, u64, vp, u64, vp, vp]
    L.spz_amd_plane_hypotheses.restype = i32
    L.spz_amd_plane_hypotheses.argtypes = [u64, u32, u32, u64, vp, dp, C.c_double, vp, pp]
    L.spz_amd_plane_score_device.restype = i32
    L.spz_amd_plane_score_device.argtypes = [vp, u64, u64, vp, u32, u64, vp, vp]
    L.spz_amd_plane_moments_device.restype = i32
    L.spz_amd_plane_moments_device.argtypes = [vp, u64, u64, pp, u64, vp, vp]
    L.spz_amd_plane_solve.restype = i32
    L.spz_amd_plane_solve.argtypes = [C.POINTER(PlaneMoments), pp, dp, dp, C.POINTER(i32)]
    L.spz_amd_plane_mark_device.restype = i32
    L.spz_amd_plane_mark_device.argtypes = [vp, u64, u64, pp, u64, C.c_uint8, vp, vp]
    L.spz_amd_plane_placement.restype = i32
    L.spz_amd_plane_placement.argtypes = [pp, i32, i32, i32, C.POINTER(PlaneResult)]
    L.spz_amd_plane_sides_host.restype = i32
    L.spz_amd_plane_sides_host.argtypes = [vp, C.c_size_t, C.POINTER(Header), pp, u64, i32, vp]
    L.spz_amd_plane_host.restype = i32
    L.spz_amd_plane_host.argtypes = [vp, C.c_size_t, C.POINTER(Header), C.POINTER(PlaneOptions), i32,
                                     C.POINTER(PlaneResult), u32, C.POINTER(u32), vp, C.POINTER(C.c_float)]
    L.spz_amd_render_check_params.restype = i32
    L.spz_amd_render_check_params.argtypes = [C.POINTER(RenderParams)]
    L.spz_amd_render_workspace_bytes.restype = u64
    L.spz_amd_render_workspace_bytes.argtypes = [u64, u64]
    L.spz_amd_render_prepare_packed_device.restype = i32
    L.spz_amd_render_prepare_packed_device.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), vp, vp, vp,
                                                       vp]
    L.spz_amd_render_prepare_cloud_device.restype = i32
    L.spz_amd_render_prepare_cloud_device.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), vp,
                                                      vp, vp, vp]
    L.spz_amd_render_finish_device.restype = i32
    L.spz_amd_render_finish_device.argtypes = [u64, C.POINTER(RenderParams), u64, vp, vp, vp, vp]
    L.spz_amd_render_host.restype = i32
    L.spz_amd_render_host.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), i32, vp, C.POINTER(u64), vp]
    L.spz_amd_render_cloud_host.restype = i32
    L.spz_amd_render_cloud_host.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), i32, vp,
                                            C.POINTER(u64), vp]
    L.spz_amd_render_score_device.restype = i32
    L.spz_amd_render_score_device.argtypes = [u64, C.POINTER(RenderParams), u64, vp, vp, vp, vp, vp, vp]
    L.spz_amd_render_depth_device.restype = i32
    L.spz_amd_render_depth_device.argtypes = [u64, C.POINTER(RenderParams), u64, vp, vp, vp, vp, vp, vp]
    L.spz_amd_render_backward_workspace_bytes.restype = u64
    L.spz_amd_render_backward_workspace_bytes.argtypes = [u64]
    L.spz_amd_render_backward_device.restype = i32
    L.spz_amd_render_backward_device.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), u64, vp, vp,
                                                 C.POINTER(CloudPtrs), vp, vp, vp, vp, vp]
    L.spz_amd_render_depth_backward_workspace_bytes.restype = u64
    L.spz_amd_render_depth_backward_workspace_bytes.argtypes = [u64]
    L.spz_amd_render_depth_backward_device.restype = i32
    L.spz_amd_render_depth_backward_device.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), u64,
                                                       vp, vp, C.POINTER(CloudPtrs), vp, vp, vp, vp, vp, vp]
    L.spz_amd_depth_loss_workspace_bytes.restype = u64
    L.spz_amd_depth_loss_workspace_bytes.argtypes = [i32, i32]
    L.spz_amd_depth_loss_device.restype = i32
    L.spz_amd_depth_loss_device.argtypes = [vp, vp, vp, vp, i32, i32, i32, C.c_float, C.c_double, vp, vp, vp, vp, vp]
    L.spz_amd_render_depth_host.restype = i32
    L.spz_amd_render_depth_host.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), i32, vp, vp, vp,
                                            C.POINTER(u64), vp]
    L.spz_amd_render_depth_cloud_host.restype = i32
    L.spz_amd_render_depth_cloud_host.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), i32, vp,
                                                  vp, vp, C.POINTER(u64), vp]
    L.spz_amd_prune_keep_count.restype = i32
    L.spz_amd_prune_keep_count.argtypes = [u64, i32, C.c_double, C.POINTER(u64)]
    L.spz_amd_prune_open.restype = i32
    L.spz_amd_prune_open.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), i32, i32, i32, C.c_double, i32,
                                     C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), vp, vp, vp, vp,
                                     C.POINTER(C.c_int32)]
    L.spz_amd_prune_fetch.restype = i32
    L.spz_amd_prune_fetch.argtypes = [vp, vp]
    L.spz_amd_prune_device_data.restype = vp
    L.spz_amd_prune_device_data.argtypes = [vp]
    L.spz_amd_prune_close.restype = None
    L.spz_amd_prune_close.argtypes = [vp]
    L.spz_amd_image_metrics_check.restype = i32
    L.spz_amd_image_metrics_check.argtypes = [i32, i32, i32, i32]
    L.spz_amd_image_metrics_workspace_bytes.restype = u64
    L.spz_amd_image_metrics_workspace_bytes.argtypes = [i32, i32]
    L.spz_amd_image_metrics_device.restype = i32
    L.spz_amd_image_metrics_device.argtypes = [vp, i32, vp, i32, i32, i32, vp, vp, vp, vp]
    L.spz_amd_image_metrics_host.restype = i32
    L.spz_amd_image_metrics_host.argtypes = [vp, i32, vp, i32, i32, i32, i32, C.POINTER(ImageMetrics), vp]
    L.spz_amd_compare_host.restype = i32
    L.spz_amd_compare_host.argtypes = [vp, sz, C.POINTER(Header), vp, sz, C.POINTER(Header), C.POINTER(RenderParams),
                                       i32, i32, C.POINTER(ImageMetrics), vp, vp, vp, C.POINTER(C.c_int32)]
    L.spz_amd_zlib_encode_blocks.restype = i32
    L.spz_amd_zlib_encode_blocks.argtypes = [vp, vp, u32, u32, vp, vp, vp, u64, u64, vp, vp]
    L.spz_amd_image_loss_workspace_bytes.restype = u64
    L.spz_amd_image_loss_workspace_bytes.argtypes = [i32, i32]
    L.spz_amd_image_loss_device.restype = i32
    L.spz_amd_image_loss_device.argtypes = [vp, i32, vp, i32, i32, i32, C.c_double, vp, vp, vp, vp]
    L.spz_amd_adam_scalars_of.restype = i32
    L.spz_amd_adam_scalars_of.argtypes = [i32, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double,
                                          C.POINTER(AdamScalars)]
    L.spz_amd_adam_step_device.restype = i32
    L.spz_amd_adam_step_device.argtypes = [C.POINTER(CloudPtrs), C.POINTER(CloudPtrs), C.POINTER(CloudPtrs),
                                           C.POINTER(CloudPtrs), u64, i32, u32, AdamScalars, vp, vp]
    L.spz_amd_refine_default_options.restype = i32
    L.spz_amd_refine_default_options.argtypes = [C.POINTER(RefineOptions)]
    L.spz_amd_refine_check.restype = i32
    L.spz_amd_refine_check.argtypes = [C.POINTER(RefineOptions)]
    L.spz_amd_refine_open.restype = i32
    L.spz_amd_refine_open.argtypes = [vp, sz, C.POINTER(Header), vp, sz, C.POINTER(Header), C.POINTER(RenderParams), i32,
                                      C.POINTER(RefineOptions), i32, C.POINTER(vp), C.POINTER(u64), vp,
                                      C.POINTER(ImageMetrics), C.POINTER(ImageMetrics), C.POINTER(u64), vp,
                                      C.POINTER(C.c_int32)]
    L.spz_amd_refine_fetch.restype = i32
    L.spz_amd_refine_fetch.argtypes = [vp, vp]
    L.spz_amd_refine_device_data.restype = vp
    L.spz_amd_refine_device_data.argtypes = [vp]
    L.spz_amd_refine_close.restype = None
    L.spz_amd_refine_close.argtypes = [vp]
    L.spz_amd_densify_default_options.restype = i32
    L.spz_amd_densify_default_options.argtypes = [C.POINTER(DensifyOptions)]
    L.spz_amd_densify_check.restype = i32
    L.spz_amd_densify_check.argtypes = [C.POINTER(DensifyOptions)]
    L.spz_amd_densify_thresholds.restype = i32
    L.spz_amd_densify_thresholds.argtypes = [C.POINTER(DensifyOptions), C.POINTER(RenderParams), i32,
                                             C.POINTER(DensifyLimits)]
    L.spz_amd_densify_accumulate_device.restype = i32
    L.spz_amd_densify_accumulate_device.argtypes = [vp, vp, u64, u32, u32, vp, vp, vp]
    L.spz_amd_densify_plan_workspace_bytes.restype = u64
    L.spz_amd_densify_plan_workspace_bytes.argtypes = [u64]
    L.spz_amd_densify_plan_device.restype = i32
    L.spz_amd_densify_plan_device.argtypes = [vp, vp, vp, vp, u64, C.POINTER(DensifyLimits), u64, u64, vp, vp, vp, vp,
                                              vp, vp]
    L.spz_amd_densify_plan_host.restype = i32
    L.spz_amd_densify_plan_host.argtypes = [vp, vp, vp, vp, u64, C.POINTER(DensifyLimits), u64, u64, vp, vp, vp, vp, vp,
                                            C.POINTER(u64), vp]
    L.spz_amd_densify_apply_device.restype = i32
    L.spz_amd_densify_apply_device.argtypes = [C.POINTER(CloudPtrs)] * 6 + [vp, vp, u64, u64, u64, i32, u64, u32, vp]
    L.spz_amd_densify_reset_opacity_device.restype = i32
    L.spz_amd_densify_reset_opacity_device.argtypes = [vp, vp, vp, u64, vp]
    L.spz_amd_refine_densify_open.restype = i32
    L.spz_amd_refine_densify_open.argtypes = [vp, sz, C.POINTER(Header), vp, sz, C.POINTER(Header),
                                              C.POINTER(RenderParams), i32, C.POINTER(RefineOptions),
                                              C.POINTER(DensifyOptions), i32, C.POINTER(vp), C.POINTER(u64), vp,
                                              C.POINTER(ImageMetrics), C.POINTER(ImageMetrics), C.POINTER(u64), vp,
                                              C.POINTER(C.c_int32), C.POINTER(u64), C.POINTER(DensifyRound), i32,
                                              C.POINTER(C.c_int32), vp]
    L.spz_amd_photo_loss_workspace_bytes.restype = u64
    L.spz_amd_photo_loss_workspace_bytes.argtypes = [i32, i32]
    L.spz_amd_photo_loss_device.restype = i32
    L.spz_amd_photo_loss_device.argtypes = [vp, i32, vp, i32, vp, C.POINTER(C.c_double), i32, i32, C.c_double, vp, vp,
                                            vp, vp, vp]
    L.spz_amd_image_exposure_device.restype = i32
    L.spz_amd_image_exposure_device.argtypes = [vp, i32, C.POINTER(C.c_double), i32, i32, vp, vp]
    L.spz_amd_photo_default_options.restype = i32
    L.spz_amd_photo_default_options.argtypes = [C.POINTER(PhotoOptions)]
    L.spz_amd_photo_check.restype = i32
    L.spz_amd_photo_check.argtypes = [C.POINTER(PhotoOptions)]
    L.spz_amd_refine_images_open.restype = i32
    L.spz_amd_refine_images_open.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), i32,
                                             C.POINTER(vp), i32, C.POINTER(vp), C.POINTER(RefineOptions),
                                             C.POINTER(PhotoOptions), C.POINTER(DensifyOptions), i32, C.POINTER(vp),
                                             C.POINTER(u64), vp, C.POINTER(ImageMetrics), C.POINTER(ImageMetrics),
                                             C.POINTER(u64), vp, C.POINTER(C.c_int32), C.POINTER(u64),
                                             C.POINTER(DensifyRound), i32, C.POINTER(C.c_int32), vp, vp]
    L.spz_amd_refine_images_host_open.restype = i32
    L.spz_amd_refine_images_host_open.argtypes = L.spz_amd_refine_images_open.argtypes
    L.spz_amd_depth_default_options.restype = i32
    L.spz_amd_depth_default_options.argtypes = [C.POINTER(DepthOptions)]
    L.spz_amd_depth_check.restype = i32
    L.spz_amd_depth_check.argtypes = [C.POINTER(DepthOptions)]
    base = L.spz_amd_refine_images_open.argtypes  # two more after the weights, two more at the end
    L.spz_amd_refine_images_depth_open.restype = i32
    L.spz_amd_refine_images_depth_open.argtypes = base[:8] + [C.POINTER(vp), C.POINTER(DepthOptions)] + base[8:] + [vp, vp]
    L.spz_amd_refine_images_depth_host_open.restype = i32
    L.spz_amd_refine_images_depth_host_open.argtypes = L.spz_amd_refine_images_depth_open.argtypes
    L.spz_amd_render_records_backward_device.restype = i32
    L.spz_amd_render_records_backward_device.argtypes = [u64, C.POINTER(RenderParams), u64, vp, vp, vp, vp, vp]
    L.spz_amd_render_view_backward_workspace_bytes.restype = u64
    L.spz_amd_render_view_backward_workspace_bytes.argtypes = [u64]
    L.spz_amd_render_view_backward_device.restype = i32
    L.spz_amd_render_view_backward_device.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), u64,
                                                      vp, vp, vp, vp, vp, vp]
    L.spz_amd_locate_default_options.restype = i32
    L.spz_amd_locate_default_options.argtypes = [C.POINTER(LocateOptions)]
    L.spz_amd_locate_check.restype = i32
    L.spz_amd_locate_check.argtypes = [C.POINTER(LocateOptions)]
    L.spz_amd_locate_level_params.restype = i32
    L.spz_amd_locate_level_params.argtypes = [C.POINTER(RenderParams), i32, C.POINTER(RenderParams)]
    L.spz_amd_locate_twist_gradient.restype = i32
    L.spz_amd_locate_twist_gradient.argtypes = [C.POINTER(C.c_double)] * 3
    L.spz_amd_locate_pose_step.restype = i32
    L.spz_amd_locate_pose_step.argtypes = [C.POINTER(LocateOptions), i32] + [C.POINTER(C.c_double)] * 4
    L.spz_amd_image_halve_device.restype = i32
    L.spz_amd_image_halve_device.argtypes = [vp, i32, i32, i32, vp, vp]
    L.spz_amd_locate_host.restype = i32
    L.spz_amd_locate_host.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), vp, i32,
                                      C.POINTER(LocateOptions), i32, vp, vp, C.POINTER(ImageMetrics),
                                      C.POINTER(ImageMetrics), C.POINTER(C.c_int32), vp]
    L.spz_amd_locate_image_host.restype = i32
    L.spz_amd_locate_image_host.argtypes = L.spz_amd_locate_host.argtypes
    L.spz_amd_locate_cloud_host.restype = i32
    L.spz_amd_locate_cloud_host.argtypes = [C.POINTER(CloudPtrs), u64, i32, i32, C.POINTER(RenderParams), vp, i32,
                                            C.POINTER(LocateOptions), i32, vp, vp, C.POINTER(ImageMetrics),
                                            C.POINTER(ImageMetrics), C.POINTER(C.c_int32), vp]
    L.spz_amd_tsdf_check.restype = i32
    L.spz_amd_tsdf_check.argtypes = [C.POINTER(TsdfVolume)]
    L.spz_amd_tsdf_bytes.restype = u64
    L.spz_amd_tsdf_bytes.argtypes = [C.POINTER(TsdfVolume)]
    L.spz_amd_tsdf_volume_from_box.restype = i32
    L.spz_amd_tsdf_volume_from_box.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.c_double,
                                               C.POINTER(TsdfVolume)]
    L.spz_amd_tsdf_integrate_device.restype = i32
    L.spz_amd_tsdf_integrate_device.argtypes = [C.POINTER(TsdfVolume), vp, C.POINTER(RenderParams), vp, vp, i32,
                                                C.c_float, vp]
    L.spz_amd_mesh_tet_table.restype = i32
    L.spz_amd_mesh_tet_table.argtypes = [vp, vp, vp]
    L.spz_amd_mesh_workspace_bytes.restype = u64
    L.spz_amd_mesh_workspace_bytes.argtypes = [C.POINTER(TsdfVolume)]
    L.spz_amd_mesh_count_device.restype = i32
    L.spz_amd_mesh_count_device.argtypes = [C.POINTER(TsdfVolume), vp, C.c_float, vp, vp, vp]
    L.spz_amd_mesh_emit_device.restype = i32
    L.spz_amd_mesh_emit_device.argtypes = [C.POINTER(TsdfVolume), vp, u64, u64, u64, u64, vp, vp, vp, vp, vp]
    L.spz_amd_mesh_default_options.restype = i32
    L.spz_amd_mesh_default_options.argtypes = [C.POINTER(MeshOptions)]
    L.spz_amd_mesh_check.restype = i32
    L.spz_amd_mesh_check.argtypes = [C.POINTER(MeshOptions)]
    L.spz_amd_mesh_open.restype = i32
    L.spz_amd_mesh_open.argtypes = [vp, sz, C.POINTER(Header), C.POINTER(RenderParams), i32, C.POINTER(MeshOptions), i32,
                                    C.POINTER(vp), C.POINTER(u64), C.POINTER(TsdfVolume), vp, C.POINTER(C.c_int32)]
    L.spz_amd_mesh_fetch.restype = i32
    L.spz_amd_mesh_fetch.argtypes = [vp, vp, vp, vp]
    L.spz_amd_mesh_close.restype = None
    L.spz_amd_mesh_close.argtypes = [vp]
    L.spz_amd_seed_default_options.restype = i32
    L.spz_amd_seed_default_options.argtypes = [C.POINTER(SeedOptions)]
    L.spz_amd_seed_check.restype = i32
    L.spz_amd_seed_check.argtypes = [C.POINTER(SeedOptions)]
    L.spz_amd_seed_samples.restype = u64
    L.spz_amd_seed_samples.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.spz_amd_seed_workspace_bytes.restype = u64
    L.spz_amd_seed_workspace_bytes.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.spz_amd_seed_view_device.restype = i32
    L.spz_amd_seed_view_device.argtypes = [C.POINTER(CloudPtrs), u64, u64, i32, C.POINTER(RenderParams),
                                           C.POINTER(SeedOptions), vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.spz_amd_seed_open.restype = i32
    L.spz_amd_seed_open.argtypes = [C.POINTER(RenderParams), i32, C.POINTER(SeedOptions), C.POINTER(vp),
                                    C.POINTER(C.c_int32), C.POINTER(vp), C.POINTER(vp), vp, sz, C.POINTER(Header), u64,
                                    i32, C.POINTER(vp), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64), vp,
                                    C.POINTER(C.c_int32)]
    L.spz_amd_seed_fetch.restype = i32
    L.spz_amd_seed_fetch.argtypes = [vp, vp]
    L.spz_amd_seed_device_data.restype = vp
    L.spz_amd_seed_device_data.argtypes = [vp]
    L.spz_amd_seed_close.restype = None
    L.spz_amd_seed_close.argtypes = [vp]
    return L


def status_string(status):
    return load_library().spz_amd_status_string(int(status)).decode()


def check(status, where):
    if status != OK:
        raise SpzAmdError(status, where)


def stream_layout(num_points, sh_degree, version=3):
    lay = Layout()
    check(load_library().spz_amd_stream_layout(int(num_points), int(sh_degree), int(version), C.byref(lay)),
          "spz_amd_stream_layout")
    return lay


def write_header(version, num_points, sh_degree, fractional_bits=12, antialiased=False):
    h = Header(int(version), int(num_points), int(sh_degree), int(fractional_bits), 1 if antialiased else 0, 0)
    out = (C.c_uint8 * 16)()
    check(load_library().spz_amd_write_header(C.byref(h), out), "spz_amd_write_header")
    return bytes(out)


def peek_header(stream_bytes, max_points=REFERENCE_MAX_POINTS):
    """stream_bytes: bytes-like HOST data (at least the header; the full stream for the size check).
    Returns (status, Header or None)."""
    buf = (C.c_uint8 * len(stream_bytes)).from_buffer_copy(stream_bytes) if len(stream_bytes) else None
    h = Header()
    rc = load_library().spz_amd_peek_header_ex(buf, len(stream_bytes), int(max_points), C.byref(h))
    return rc, (h if rc == OK else None)


def transform_params(rotation=None, translation=None, scale=1.0, coord=UNSPECIFIED):
    """The f32 parameter block of p -> scale * R(rotation) * p + translation stated in `coord` (spz_amd_transform_params,
    host only).  rotation (x, y, z, w): None = identity; translation: None = 0.  A bad argument raises ValueError."""
    import math
    dbl = C.c_double
    q = t = None
    if rotation is not None:
        rotation = [float(v) for v in rotation]
        if len(rotation) != 4:
            raise ValueError("rotation must be (x, y, z, w)")
        q = (dbl * 4)(*rotation)
    if translation is not None:
        translation = [float(v) for v in translation]
        if len(translation) != 3:
            raise ValueError("translation must be (x, y, z)")
        t = (dbl * 3)(*translation)
    if isinstance(scale, bool) or not isinstance(scale, (int, float)) or not math.isfinite(scale):
        raise ValueError("scale must be a finite number > 0")
    out = Transform()
    rc = load_library().spz_amd_transform_params(q, t, float(scale), int(coord), C.byref(out))
    if rc != OK:
        raise ValueError(f"invalid transform: rotation={rotation} translation={translation} scale={scale} coord={coord}")
    return out


def render_params(world_to_camera, fx, fy, cx, cy, width, height, near=0.2, background=(0.0, 0.0, 0.0),
                  max_sh_degree=3, coord=UNSPECIFIED):
    """A RenderParams, checked on the host (spz_amd_render_check_params): ValueError on a bad camera or size."""
    import numpy as np
    m = np.asarray(world_to_camera, dtype=np.float64)
    if m.shape != (3, 4):
        raise ValueError(f"world_to_camera must be 3x4, got shape {m.shape}")
    bg = np.asarray(background, dtype=np.float64).reshape(-1)
    if bg.size != 3:
        raise ValueError("background must have three values")
    for name, v in (("width", width), ("height", height), ("max_sh_degree", max_sh_degree), ("coord", coord)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise ValueError(f"{name} must be an int, got {v!r}")
    if not (1 <= width <= 16384 and 1 <= height <= 16384):
        raise ValueError(f"width and height must be in 1..16384, got {width} x {height}")
    p = RenderParams()
    for k, v in enumerate(m.reshape(-1)):
        p.world_to_camera[k] = float(v)
    p.fx, p.fy, p.cx, p.cy = float(fx), float(fy), float(cx), float(cy)
    p.width, p.height = width, height
    p.near_plane = float(near)
    for k in range(3):
        p.background[k] = float(bg[k])
    p.max_sh_degree, p.coord = max_sh_degree, coord
    if load_library().spz_amd_render_check_params(C.byref(p)) != OK:
        raise ValueError("bad render parameters: world_to_camera must be [R | t] with R a rotation (to 1e-4), fx, fy > 0, "
                         "near > 0, everything finite, max_sh_degree 0..3, coord 0..8")
    return p


def train_mask(arrays):
    """The six-bit mask of an iterable of array names (TRAIN_ARRAYS), or an int that already is one."""
    if isinstance(arrays, int) and not isinstance(arrays, bool):
        mask = arrays
    else:
        mask = 0
        for k in arrays:
            if k not in TRAIN_ARRAYS:
                raise ValueError(f"train: unknown array {k!r} (one of {', '.join(TRAIN_ARRAYS)})")
            mask |= 1 << TRAIN_ARRAYS.index(k)
    if not 0 < mask <= TRAIN_ALL:
        raise ValueError("train: at least one array, and only the six")
    return mask


def adam_scalars(t, lrs, beta1=0.9, beta2=0.999, eps=1e-15):
    """The f32 scalars of Adam step t >= 1 (spz_amd_adam_scalars_of): lrs, six learning rates in TRAIN_ARRAYS' order."""
    out = AdamScalars()
    check(load_library().spz_amd_adam_scalars_of(int(t), (C.c_double * 6)(*[float(x) for x in lrs]), float(beta1),
                                                 float(beta2), float(eps), C.byref(out)), "spz_amd_adam_scalars_of")
    return out


def refine_options(iterations, *, lambda_dssim=None, lrs=None, beta1=None, beta2=None, eps=None, train=None):
    """spz_amd_refine_default_options with the given fields replaced.  lrs: a dict by array name or six numbers."""
    o = RefineOptions()
    check(load_library().spz_amd_refine_default_options(C.byref(o)), "spz_amd_refine_default_options")
    if isinstance(iterations, bool) or not isinstance(iterations, int):
        raise ValueError(f"iterations must be an int, got {iterations!r}")
    o.iterations = iterations
    if lambda_dssim is not None:
        o.lambda_dssim = float(lambda_dssim)
    if lrs is not None:
        if isinstance(lrs, dict):
            for k, x in lrs.items():
                o.lr[TRAIN_ARRAYS.index(k)] = float(x)
        else:
            for k, x in enumerate(lrs):
                o.lr[k] = float(x)
    for name, x in (("beta1", beta1), ("beta2", beta2), ("eps", eps)):
        if x is not None:
            setattr(o, name, float(x))
    if train is not None:
        o.train_mask = train_mask(train)
    return o


def photo_options(fit_exposure=False, lr_exposure=None):
    """spz_amd_photo_default_options with the given fields replaced, checked by spz_amd_photo_check: ValueError on a
    refused value."""
    L = load_library()
    o = PhotoOptions()
    check(L.spz_amd_photo_default_options(C.byref(o)), "spz_amd_photo_default_options")
    if not isinstance(fit_exposure, (bool, int)):
        raise ValueError(f"fit_exposure must be a bool, got {fit_exposure!r}")
    o.fit_exposure = 1 if fit_exposure else 0
    if lr_exposure is not None:
        o.lr_exposure = float(lr_exposure)
    if L.spz_amd_photo_check(C.byref(o)) != OK:
        raise ValueError(f"lr_exposure must be a finite number >= 0, got {lr_exposure!r}")
    return o


def depth_options(weight=None, kind=None, min_alpha=None):
    """spz_amd_depth_default_options with the given fields replaced (kind: "l1" or "inverse"), checked by
    spz_amd_depth_check: ValueError on a refused value."""
    L = load_library()
    o = DepthOptions()
    check(L.spz_amd_depth_default_options(C.byref(o)), "spz_amd_depth_default_options")
    if weight is not None:
        o.weight = float(weight)
    if kind is not None:
        if kind not in ("l1", "inverse"):
            raise ValueError(f"depth_kind must be 'l1' or 'inverse', got {kind!r}")
        o.kind = DEPTH_L1 if kind == "l1" else DEPTH_INVERSE_L1
    if min_alpha is not None:
        o.min_alpha = float(min_alpha)
    if L.spz_amd_depth_check(C.byref(o)) != OK:
        raise ValueError(f"depth_weight must be finite and >= 0 and depth_min_alpha in (0, 1], got {weight!r} and "
                         f"{min_alpha!r}")
    return o


def exposure_values(exposure):
    """The 12 doubles [M | o], row-major, of a (3, 4) array-like (or 12 numbers) as a ctypes array: ValueError when
    it has another size or a value is not finite."""
    import numpy as np
    e = np.asarray(exposure, dtype=np.float64).reshape(-1)
    if e.size != 12 or not np.isfinite(e).all():
        raise ValueError("exposure must be 12 finite numbers, a row-major 3 x 4 [M | o]")
    return (C.c_double * 12)(*e.tolist())


LOCATE_FIELDS = ("iterations", "levels", "lambda_dssim", "lr_rotation", "lr_translation", "lr_final_factor", "beta1",
                 "beta2", "eps")


def locate_options(**fields):
    """spz_amd_locate_default_options with the given fields (LOCATE_FIELDS) replaced, checked by spz_amd_locate_check:
    ValueError on an unknown field or a refused value."""
    L = load_library()
    o = LocateOptions()
    check(L.spz_amd_locate_default_options(C.byref(o)), "spz_amd_locate_default_options")
    for k, x in fields.items():
        if k not in LOCATE_FIELDS:
            raise ValueError(f"locate: unknown option {k!r} (one of {', '.join(LOCATE_FIELDS)})")
        if x is None:
            continue
        if k in ("iterations", "levels"):
            if isinstance(x, bool) or not isinstance(x, int):
                raise ValueError(f"{k} must be an int, got {x!r}")
            setattr(o, k, x)
        else:
            setattr(o, k, float(x))
    if L.spz_amd_locate_check(C.byref(o)) != OK:
        raise ValueError("bad locate options: iterations >= 0, levels 1..8, lambda_dssim in [0, 1], step sizes >= 0, "
                         "lr_final_factor in (0, 1], beta1, beta2 in [0, 1), eps >= 0")
    return o


def locate_level_params(params, level):
    """The view of coarse-to-fine level `level` (spz_amd_locate_level_params): the size and fx, fy, cx, cy divided by
    2^level.  ValueError when the size is not divisible."""
    out = RenderParams()
    if load_library().spz_amd_locate_level_params(C.byref(params), int(level), C.byref(out)) != OK:
        raise ValueError(f"level {level}: width and height must be divisible by 2^level (level 0..7)")
    return out


def tsdf_volume(lo, dims, voxel_size, truncation=None):
    """A TsdfVolume, checked on the host (spz_amd_tsdf_check): ValueError when refused.  truncation: None = 4 voxels."""
    v = TsdfVolume()
    lo, dims = [float(x) for x in lo], [int(x) for x in dims]
    if len(lo) != 3 or len(dims) != 3 or min(dims) < 0 or max(dims) > 2**32 - 1:
        raise ValueError("lo and dims must have three values each")
    for a in range(3):
        v.lo[a], v.dims[a] = lo[a], dims[a]
    v.voxel_size = float(voxel_size)
    v.truncation = 4.0 * float(voxel_size) if truncation is None else float(truncation)
    if load_library().spz_amd_tsdf_check(C.byref(v)) != OK:
        raise ValueError("bad volume: each dimension 2..2048, at most 2^28 lattice points, voxel_size and truncation "
                         "finite and > 0, lo finite")
    return v


def tsdf_volume_from_box(lo, hi, voxel_size, truncation=None):
    """The TsdfVolume that covers the box lo..hi at `voxel_size` (spz_amd_tsdf_volume_from_box): dims_a =
    floor((hi_a - lo_a) / voxel_size) + 2.  ValueError when refused."""
    lo, hi = [float(x) for x in lo], [float(x) for x in hi]
    if len(lo) != 3 or len(hi) != 3:
        raise ValueError("lo and hi must have three values each")
    v = TsdfVolume()
    t = 4.0 * float(voxel_size) if truncation is None else float(truncation)
    if load_library().spz_amd_tsdf_volume_from_box((C.c_double * 3)(*lo), (C.c_double * 3)(*hi), float(voxel_size), t,
                                                   C.byref(v)) != OK:
        raise ValueError("bad box or voxel size: hi >= lo, everything finite, voxel_size and truncation > 0, each "
                         "dimension at most 2048 and at most 2^28 lattice points")
    return v


def mesh_tet_table():
    """The generated marching-tetrahedra table (spz_amd_mesh_tet_table, host only): corners (6, 4), num_triangles
    (6, 16) and edges (6, 16, 6) as uint8 arrays."""
    import numpy as np
    c, n, e = np.zeros((6, 4), np.uint8), np.zeros((6, 16), np.uint8), np.zeros((6, 16, 6), np.uint8)
    check(load_library().spz_amd_mesh_tet_table(c.ctypes.data, n.ctypes.data, e.ctypes.data), "spz_amd_mesh_tet_table")
    return c, n, e


MESH_FIELDS = ("box", "voxel_size", "resolution", "truncation", "depth", "min_alpha", "min_weight")


def mesh_options(**fields):
    """spz_amd_mesh_default_options with the given fields (MESH_FIELDS) replaced, checked by spz_amd_mesh_check:
    ValueError on an unknown field or a refused value.  voxel_size and resolution exclude each other; with neither,
    resolution = 256."""
    L = load_library()
    o = MeshOptions()
    check(L.spz_amd_mesh_default_options(C.byref(o)), "spz_amd_mesh_default_options")
    for k in fields:
        if k not in MESH_FIELDS:
            raise ValueError(f"mesh: unknown option {k!r} (one of {', '.join(MESH_FIELDS)})")
    f = {k: x for k, x in fields.items() if x is not None}
    if "voxel_size" in f and "resolution" in f:
        raise ValueError("mesh: voxel_size and resolution exclude each other")
    if "box" in f:
        box = [float(x) for x in f["box"]]
        if len(box) != 6:
            raise ValueError("mesh: box must be (x0, y0, z0, x1, y1, z1)")
        o.has_box = 1
        for a in range(6):
            o.box[a] = box[a]
    if "voxel_size" in f:
        o.voxel_size, o.resolution = float(f["voxel_size"]), 0
        if o.voxel_size == 0.0:
            raise ValueError("mesh: voxel_size must be > 0")
    if "resolution" in f:
        x = f["resolution"]
        if isinstance(x, bool) or not isinstance(x, int) or not 1 <= x <= 2046:
            raise ValueError(f"mesh: resolution must be an int in 1..2046, got {x!r}")
        o.resolution = x
    if "truncation" in f:
        o.truncation = float(f["truncation"])
        if o.truncation == 0.0:
            raise ValueError("mesh: truncation must be > 0")
    if "depth" in f:
        if f["depth"] not in MESH_DEPTH_KINDS:
            raise ValueError(f"mesh: depth must be 'median' or 'expected', got {f['depth']!r}")
        o.depth_kind = MESH_DEPTH_KINDS[f["depth"]]
    for k in ("min_alpha", "min_weight"):
        if k in f:
            setattr(o, k, float(f[k]))
    if L.spz_amd_mesh_check(C.byref(o)) != OK:
        raise ValueError("mesh: refused options (box hi > lo and finite, voxel_size > 0 or resolution 1..2046, "
                         "truncation > 0, min_alpha in [0, 1], min_weight > 0)")
    return o


SEED_FIELDS = ("stride", "scale_factor", "opacity", "cover", "cover_alpha", "cover_tolerance", "sh_degree")


def seed_alpha(opacity):
    """The pre-sigmoid alpha of an opacity in (0, 1): log(o / (1 - o)) in f64, rounded to f32 by the options struct; 0.5
    gives exactly 0.  ValueError outside (0, 1)."""
    import math
    o = float(opacity)
    if not 0.0 < o < 1.0:
        raise ValueError(f"seed: opacity must be in (0, 1), got {opacity!r}")
    return math.log(o / (1.0 - o))


def seed_options(**fields):
    """spz_amd_seed_default_options with the given fields (SEED_FIELDS) replaced, checked by spz_amd_seed_check:
    ValueError on an unknown field or a refused value.  opacity in (0, 1) becomes the struct's pre-sigmoid alpha."""
    L = load_library()
    o = SeedOptions()
    check(L.spz_amd_seed_default_options(C.byref(o)), "spz_amd_seed_default_options")
    for k in fields:
        if k not in SEED_FIELDS:
            raise ValueError(f"seed: unknown option {k!r} (one of {', '.join(SEED_FIELDS)})")
    f = {k: x for k, x in fields.items() if x is not None}
    for k in ("stride", "sh_degree"):
        if k in f:
            x = f[k]
            if isinstance(x, bool) or not isinstance(x, int) or not 0 <= x <= 2**31 - 1:
                raise ValueError(f"seed: {k} must be a non-negative int, got {x!r}")
            setattr(o, k, x)
    if "opacity" in f:
        o.alpha = seed_alpha(f["opacity"])
    if "cover" in f:
        o.cover = 1 if f["cover"] else 0
    for k in ("scale_factor", "cover_alpha", "cover_tolerance"):
        if k in f:
            setattr(o, k, float(f[k]))
    if L.spz_amd_seed_check(C.byref(o)) != OK:
        raise ValueError("seed: refused options (stride 1..64, scale_factor > 0, opacity in (0, 1), cover_alpha in "
                         "[0, 1], cover_tolerance >= 0, sh_degree 0..3)")
    return o


def seed_samples(width, height, stride=1):
    """The number of lattice samples of a width x height view at `stride` (spz_amd_seed_samples, host only)."""
    return int(load_library().spz_amd_seed_samples(int(width), int(height), int(stride)))


def densify_options(options=None, **fields):
    """spz_amd_densify_default_options with the given fields replaced (a dict, a DensifyOptions to copy, or keywords:
    DENSIFY_FIELDS), checked by spz_amd_densify_check: ValueError on an unknown field or a refused value."""
    L = load_library()
    o = DensifyOptions()
    check(L.spz_amd_densify_default_options(C.byref(o)), "spz_amd_densify_default_options")
    if isinstance(options, DensifyOptions):
        o = DensifyOptions.from_buffer_copy(options)
    elif options is not None:
        if not isinstance(options, dict):
            raise ValueError("densify must be a dict or an abi.DensifyOptions")
        fields = {**options, **fields}
    for k, x in fields.items():
        if k not in DENSIFY_FIELDS:
            raise ValueError(f"densify: unknown field {k!r} (one of {', '.join(DENSIFY_FIELDS)})")
        if isinstance(getattr(o, k), int):
            if isinstance(x, bool) or not isinstance(x, int) or x < 0 or (k not in ("max_points", "seed") and x > 2**31 - 1) \
                    or x > 2**64 - 1:
                raise ValueError(f"densify: {k} must be a non-negative int, got {x!r}")
            setattr(o, k, x)
        else:
            setattr(o, k, float(x))
    if L.spz_amd_densify_check(C.byref(o)) != OK:
        raise ValueError("densify: refused options (values >= 0 and finite, until_iter >= from_iter, min_opacity in "
                         "(0, 1), percent_dense > 0 when interval > 0)")
    return o


def densify_thresholds(options, views=()):
    """The f32 thresholds of `options` over `views` (spz_amd_densify_thresholds, host only): a DensifyLimits.  With
    extent == 0 it is derived from the views' camera centres; when that gives 0, SpzAmdError (invalid argument)."""
    views = list(views)
    arr = (RenderParams * max(1, len(views)))(*views)
    out = DensifyLimits()
    check(load_library().spz_amd_densify_thresholds(C.byref(options), arr if views else None, len(views), C.byref(out)),
          "spz_amd_densify_thresholds")
    return out


def merge_resolve(headers, sh_degree=None, fractional_bits=None, antialiased=None):
    """The output header and byte count of a merge of streams with these headers (spz_amd_merge_resolve, host only):
    (status, Header or None, bytes).  None = the default of each request."""
    hs = list(headers)
    arr = (Header * max(len(hs), 1))(*hs)
    out, nbytes = Header(), C.c_uint64(0)
    req = [-1 if v is None else int(v) for v in (sh_degree, fractional_bits, antialiased)]
    rc = load_library().spz_amd_merge_resolve(arr, len(hs), *req, C.byref(out), C.byref(nbytes))
    return rc, (out if rc == OK else None), int(nbytes.value)


def get_tables():
    import numpy as np
    a = np.zeros(256, np.float32)
    c = np.zeros(256, np.float32)
    t = np.zeros(255, np.float32)
    check(load_library().spz_amd_get_tables(a.ctypes.data, c.ctypes.data, t.ctypes.data), "spz_amd_get_tables")
    return a, c, t
