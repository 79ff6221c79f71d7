"""ctypes binding of libc3dgs_hip.so (include/c3dgs_hip.h).  No CPU fallback: if the HIP library is
missing or cannot be loaded, importing any op raises immediately."""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# C3DGS_LIB_PATH: test hook only -- loads a variant build of the SAME library (c3dgs_amd/build.py VARIANTS, DIAG_VARIANTS)
LIB_PATH = os.environ.get("C3DGS_LIB_PATH") or os.path.join(_HERE, "libc3dgs_hip.so")

_f32p = C.POINTER(C.c_float)
_i64p = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u8p = C.POINTER(C.c_uint8)

RESIZE_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)


class RasterParams(C.Structure):
    _fields_ = [
        ("P", C.c_int32), ("D", C.c_int32), ("M", C.c_int32), ("W", C.c_int32), ("H", C.c_int32),
        ("SHS", C.c_int32), ("GS", C.c_int32),
        ("background", C.c_void_p), ("means3D", C.c_void_p), ("sh", C.c_void_p), ("colors_precomp", C.c_void_p),
        ("opacities", C.c_void_p), ("scales", C.c_void_p), ("scale_factors", C.c_void_p), ("rotations", C.c_void_p),
        ("cov3D_precomp", C.c_void_p), ("sh_indices", C.c_void_p), ("g_indices", C.c_void_p),
        ("viewmatrix", C.c_void_p), ("projmatrix", C.c_void_p), ("campos", C.c_void_p),
        ("tan_fovx", C.c_float), ("tan_fovy", C.c_float), ("scale_modifier", C.c_float),
        ("prefiltered", C.c_int32), ("clamp_color", C.c_int32), ("debug", C.c_int32),
    ]


class RasterGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales",
        "dL_dscale_factors", "dL_drotations")]


class GeomLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "total_bytes", "splat", "depth_keys", "depth_keys_sorted", "depth_order",
        "sorted_offsets", "inst_offset", "rects", "clamped", "scan_temp", "scan_temp_bytes", "block_base", "depth_base")]


class BinningLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in (
        "total_bytes", "keys_unsorted", "values_unsorted", "keys_sorted", "point_list", "sort_temp", "sort_temp_bytes")]


class StageTime(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("total_ms", C.c_double), ("count", C.c_int64)]


class ImageLayout(C.Structure):
    _fields_ = [(n, C.c_size_t) for n in ("total_bytes", "final_T", "n_contrib", "ranges", "tile_used", "tile_order")]


class BackwardLayout(C.Structure):    # c3dgs_get_backward_layout: the backward's workspace
    _fields_ = [(n, C.c_size_t) for n in ("total_bytes", "partials", "touched", "live_ids", "live_slots", "live_count", "list_len")]


class CompactLayout(C.Structure):     # c3dgs_get_compact_layout: the compact per-tile lists the backward walks
    _fields_ = [(n, C.c_size_t) for n in ("cqm", "cid", "tile_used_c", "n_contrib_c")]


class QatParams(C.Structure):
    _fields_ = [("P", C.c_int32), ("GS", C.c_int32), ("SHS", C.c_int32), ("M", C.c_int32),
                ("xyz", C.c_void_p), ("opacity", C.c_void_p), ("scaling_factor", C.c_void_p), ("scaling", C.c_void_p),
                ("rotation", C.c_void_p), ("features_dc", C.c_void_p), ("features_rest", C.c_void_p), ("state", C.c_void_p),
                ("observer_enabled", C.c_int32 * 6), ("fake_quant_enabled", C.c_int32 * 6),
                ("half_xyz", C.c_int32), ("averaging_constant", C.c_float)]


class AdamTensor(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p), ("n", C.c_int64),
                ("step_size", C.c_float), ("bias_correction2_sqrt", C.c_float)]


class SparseAdamTensor(C.Structure):    # c3dgs_sparse_adam_tensor: AdamTensor's fields (n = P * row_len) + row_len
    _fields_ = AdamTensor._fields_ + [("row_len", C.c_int32)]


class RowsTensor(C.Structure):          # c3dgs_rows_tensor
    _fields_ = [("in_param", C.c_void_p), ("in_exp_avg", C.c_void_p), ("in_exp_avg_sq", C.c_void_p), ("out_param", C.c_void_p),
                ("out_exp_avg", C.c_void_p), ("out_exp_avg_sq", C.c_void_p), ("row_floats", C.c_int32), ("role", C.c_int32)]


class Filter3DRows(C.Structure):        # c3dgs_filter3d_rows
    _fields_ = [("n", C.c_int32), ("P_model", C.c_int32), ("opacities", C.c_void_p), ("scales", C.c_void_p), ("rotations", C.c_void_p),
                ("scale_factors", C.c_void_p), ("g_indices", C.c_void_p), ("cov3D_precomp", C.c_void_p), ("filter_3D", C.c_void_p),
                ("visible", C.c_void_p),
                ("rank", C.c_void_p), ("scale_modifier", C.c_float)]


class Filter3DGrads(C.Structure):       # c3dgs_filter3d_grads
    _fields_ = [(n, C.c_void_p) for n in ("dL_dcov3D", "dL_dopacity_out", "dL_dopacity", "dL_dscales", "dL_drotations",
                                          "dL_dscale_factors")]


class Lattice(C.Structure):             # c3dgs_lattice
    _fields_ = [("Nx", C.c_int32), ("Ny", C.c_int32), ("Nz", C.c_int32), ("ox", C.c_float), ("oy", C.c_float), ("oz", C.c_float),
                ("voxel_size", C.c_float)]


ROLE_COPY, ROLE_XYZ, ROLE_SCALING = 0, 1, 2
MCMC_ROLE_OPACITY, MCMC_ROLE_SCALE = 3, 4             # c3dgs_mcmc_apply
ROW_KEEP, ROW_CLONE, ROW_SPLIT, ROW_CHILD_KEPT = 1, 2, 4, 8

_vp = C.c_void_p
# name -> (restype, argtypes); every symbol include/c3dgs_hip.h declares, and the test hooks of include/c3dgs_hip_debug.h
PROTOTYPES = {
    "c3dgs_camera_from_pose": (C.c_int, [C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_mark_visible": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_mark_visible_pose": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_rasterize_gaussians": (C.c_int, [C.POINTER(RasterParams), RESIZE_FN, C.c_void_p, RESIZE_FN, C.c_void_p,
                                            RESIZE_FN, C.c_void_p, C.c_void_p, C.c_void_p, _i32p, C.c_void_p]),
    "c3dgs_rasterize_gaussians_indexed": (C.c_int, [C.POINTER(RasterParams), RESIZE_FN, C.c_void_p, RESIZE_FN, C.c_void_p,
                                                    RESIZE_FN, C.c_void_p, C.c_void_p, C.c_void_p, _i32p, C.c_void_p]),
    "c3dgs_rasterize_gaussians_backward": (C.c_int, [C.POINTER(RasterParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.c_int32, C.c_void_p, RESIZE_FN, C.c_void_p,
                                                     C.POINTER(RasterGrads), C.c_void_p]),
    "c3dgs_rasterize_gaussians_backward_indexed": (C.c_int, [C.POINTER(RasterParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                             C.c_void_p, C.c_int32, C.c_void_p, RESIZE_FN, C.c_void_p,
                                                             C.POINTER(RasterGrads), C.c_void_p]),
    "c3dgs_rasterize_gaussians_backward_depth": (C.c_int, [C.POINTER(RasterParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                           C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, RESIZE_FN,
                                                           C.c_void_p, C.POINTER(RasterGrads), C.c_void_p]),
    "c3dgs_rasterize_gaussians_backward_depth_indexed": (C.c_int, [C.POINTER(RasterParams), C.c_void_p, C.c_void_p, C.c_void_p,
                                                                   C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                                   RESIZE_FN, C.c_void_p, C.POINTER(RasterGrads), C.c_void_p]),
    "c3dgs_depth_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "c3dgs_render_depth": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c3dgs_render_distortion": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float, _vp, _vp,
                                          _vp]),
    "c3dgs_rasterize_gaussians_backward_distortion": (C.c_int, [C.POINTER(RasterParams), _vp, _vp, _vp, _vp, C.c_int32, _vp, _vp, _vp,
                                                                _vp, _vp, C.c_float, C.c_float, RESIZE_FN, _vp,
                                                                C.POINTER(RasterGrads), _vp]),
    "c3dgs_rasterize_gaussians_backward_distortion_indexed": (C.c_int, [C.POINTER(RasterParams), _vp, _vp, _vp, _vp, C.c_int32, _vp,
                                                                        _vp, _vp, _vp, _vp, C.c_float, C.c_float, RESIZE_FN, _vp,
                                                                        C.POINTER(RasterGrads), _vp]),
    "c3dgs_distortion_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "c3dgs_gaussian_normals": (C.c_int, [C.c_int32] + [_vp] * 7),
    "c3dgs_render_normal": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_vp] * 6),
    "c3dgs_rasterize_gaussians_backward_normal": (C.c_int, [C.POINTER(RasterParams), _vp, _vp, _vp, _vp, C.c_int32] + [_vp] * 10 +
                                                  [C.c_float, C.c_float, RESIZE_FN, _vp, C.POINTER(RasterGrads), _vp]),
    "c3dgs_rasterize_gaussians_backward_normal_indexed": (C.c_int, [C.POINTER(RasterParams), _vp, _vp, _vp, _vp, C.c_int32] +
                                                          [_vp] * 10 + [C.c_float, C.c_float, RESIZE_FN, _vp,
                                                                       C.POINTER(RasterGrads), _vp]),
    "c3dgs_normal_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "c3dgs_depth_to_normal": (C.c_int, [C.c_int32, C.c_int32, _vp, C.c_float, C.c_float, _vp, _vp]),
    "c3dgs_depth_to_normal_backward": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, C.c_float, C.c_float, _vp, _vp]),
    "c3dgs_contrib_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "c3dgs_render_contrib": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_vp] * 8),
    "c3dgs_contrib_accumulate": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 10),
    "c3dgs_error_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "c3dgs_render_error": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [_vp] * 7),
    "c3dgs_pose_grad_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_pose_grad": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_float] + [_vp] * 17),
    "c3dgs_aa_opacity": (C.c_int, [C.POINTER(RasterParams), _vp, _vp, _vp]),
    "c3dgs_aa_opacity_backward": (C.c_int, [C.POINTER(RasterParams), _vp, C.POINTER(RasterGrads), _vp]),
    "c3dgs_filter3d_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_filter3d_compute": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "c3dgs_filter3d_apply": (C.c_int, [C.POINTER(Filter3DRows), _vp, _vp, _vp]),
    "c3dgs_filter3d_apply_backward": (C.c_int, [C.POINTER(Filter3DRows), C.POINTER(Filter3DGrads), _vp]),
    "c3dgs_tsdf_integrate": (C.c_int, [C.POINTER(Lattice), C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_float, C.c_float,
                                       C.c_float, _vp, _vp, _vp, _vp]),
    "c3dgs_mesh_extract_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "c3dgs_mesh_extract_count": (C.c_int, [C.POINTER(Lattice), _vp, _vp, _vp, C.c_size_t, C.POINTER(C.c_int64), _vp]),
    "c3dgs_mesh_extract_emit": (C.c_int, [C.POINTER(Lattice), _vp, _vp, _vp, _vp, C.c_size_t, C.c_int64, C.c_int64, _vp, _vp, _vp,
                                          _vp]),
    "c3dgs_error_map_l1": (C.c_int, [C.c_int32, C.c_int32, C.c_int32] + [_vp] * 4),
    "c3dgs_error_accumulate": (C.c_int, [C.c_int32, C.c_int32] + [_vp] * 6),
    "c3dgs_weighted_distance": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "c3dgs_vq_accumulate": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_weighted_distance_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int32, C.c_int32]),
    "c3dgs_weighted_distance_ws": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c3dgs_debug_wd_scores": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_vq_sums": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c3dgs_vq_step_supported": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "c3dgs_vq_step_sums": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c3dgs_vq_step_apply": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                      C.c_float, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    "c3dgs_vq_apply": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_float,
                                 C.c_int32, C.c_void_p]),
    "c3dgs_mt19937_fill": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_void_p, C.c_int64]),
    "c3dgs_draws_to_indices": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_host_buffer_device_address": (C.c_void_p, [C.c_void_p]),
    "c3dgs_draws_upload": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_morton_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_morton_order": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "c3dgs_knn_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_knn_mean_dist2": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp]),
    "c3dgs_knn_neighbours": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "c3dgs_nn_index_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_nn_build": (C.c_int, [C.c_int32, _vp, _vp, _vp]),
    "c3dgs_nn_query_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_nn_query": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_int32, _vp, _vp, _vp, _vp, _vp]),
    "c3dgs_mesh_sample_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_mesh_sample_count": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_float, C.c_uint32, _vp, C.c_size_t,
                                          C.POINTER(C.c_uint64), _vp]),
    "c3dgs_mesh_sample_emit": (C.c_int, [C.c_int32, _vp, C.c_int32, _vp, C.c_uint32, _vp, C.c_size_t, C.c_int64, _vp, _vp, _vp]),
    "c3dgs_geometry_reduce_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "c3dgs_geometry_reduce": (C.c_int, [C.c_int64, _vp, _vp, _f32p, C.c_float, C.c_int32, _f32p, _vp, C.c_size_t, _vp, _vp]),
    "c3dgs_ray_fill_plan_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "c3dgs_ray_fill_plan": (C.c_int, [C.c_int32, _vp, C.c_float, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "c3dgs_ray_fill_xyz": (C.c_int, [C.c_int32, _vp, _vp, _vp, C.c_float, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "c3dgs_image_from_u8": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _vp, C.c_int32, _vp, C.c_int32, C.c_int32, _vp, _vp]),
    "c3dgs_adam_step": (C.c_int, [C.c_int32, C.POINTER(AdamTensor), C.c_double, C.c_double, C.c_double, _vp]),
    "c3dgs_sparse_adam_workspace_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "c3dgs_sparse_adam_select": (C.c_int, [C.c_int64, _vp, C.c_int32, _vp, _vp]),
    "c3dgs_sparse_adam_step": (C.c_int, [C.c_int32, C.POINTER(SparseAdamTensor), C.c_int64, _vp, C.c_double, C.c_double, C.c_double,
                                         _vp]),
    "c3dgs_densify_classify": (C.c_int, [C.c_int32] + [_vp] * 7 + [C.c_float] * 4 + [_vp, _vp]),
    "c3dgs_rows_plan_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_rows_plan": (C.c_int, [C.c_int32, _vp, C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "c3dgs_rows_apply": (C.c_int, [C.c_int32, C.c_int64, _vp, _vp, _vp, C.c_int32, C.POINTER(RowsTensor), C.c_int32, C.c_int64,
                                   _vp, _vp, _vp, C.c_int32, C.c_int32, _vp]),
    "c3dgs_densify_stats": (C.c_int, [C.c_int32] + [_vp] * 7),
    "c3dgs_mcmc_workspace_bytes": (C.c_int, [C.c_int64, C.POINTER(C.c_size_t)]),
    "c3dgs_mcmc_sample": (C.c_int, [C.c_int64, _vp, _vp, C.c_int32, C.c_float, _vp, C.c_int64, _vp, C.c_int32, _vp, _vp, _vp, _vp,
                                    _vp, _vp]),
    "c3dgs_mcmc_apply": (C.c_int, [C.c_int64, C.c_int64, _vp, C.c_int64, _vp, _vp, C.c_int32, C.POINTER(RowsTensor), C.c_int32,
                                   C.c_float, _vp, _vp]),
    "c3dgs_mcmc_noise": (C.c_int, [C.c_int64] + [_vp] * 6 + [C.c_float, C.c_float, _vp]),
    "c3dgs_bilagrid_workspace_bytes": (C.c_size_t, [C.c_int32] * 5),
    "c3dgs_bilagrid_slice": (C.c_int, [C.c_int32] * 5 + [_vp] * 4),
    "c3dgs_bilagrid_slice_backward": (C.c_int, [C.c_int32] * 5 + [_vp] * 7),
    "c3dgs_bilagrid_tv": (C.c_int, [C.c_int32] * 4 + [_vp] * 4),
    "c3dgs_bilagrid_tv_backward": (C.c_int, [C.c_int32] * 4 + [_vp] * 4),
    "c3dgs_index_plan_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "c3dgs_index_plan": (C.c_int, [C.c_int32, _vp, _vp, C.c_int32, _vp, C.c_int32, C.c_int64, C.c_int64, C.c_int64] + [_vp] * 8),
    "c3dgs_extract_rot_scale": (C.c_int, [C.c_int32, _vp, _vp, _vp, _vp]),
    "c3dgs_l1_ssim_forward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "c3dgs_l1_ssim_value": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_void_p, C.c_void_p]),
    "c3dgs_l1_ssim_backward": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "c3dgs_image_metrics_ws_bytes": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "c3dgs_image_metrics": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "c3dgs_qat_workspace_bytes": (C.c_size_t, []),
    "c3dgs_qat_scan_bytes": (C.c_size_t, [C.c_int32]),
    "c3dgs_qat_observe": (C.c_int, [C.POINTER(QatParams), _vp, _vp]),
    "c3dgs_qat_codebooks": (C.c_int, [C.POINTER(QatParams), _vp, _vp, _vp, _vp]),
    "c3dgs_qat_codebooks_backward": (C.c_int, [C.POINTER(QatParams)] + [_vp] * 8),
    "c3dgs_qat_visible": (C.c_int, [C.POINTER(QatParams), _vp, _vp, _vp, _vp, _vp, _vp]),
    "c3dgs_qat_points": (C.c_int, [C.POINTER(QatParams)] + [_vp] * 10),
    "c3dgs_qat_points_backward": (C.c_int, [C.POINTER(QatParams)] + [_vp] * 11),
    "c3dgs_qat_quantize": (C.c_int, [C.POINTER(QatParams), C.c_int32] + [_vp] * 7),
    "c3dgs_fake_quantize": (C.c_int, [C.c_int64, _vp, _vp, C.c_int32, C.c_int32, C.c_float, _vp, _vp, _vp]),
    "c3dgs_fake_quantize_backward": (C.c_int, [C.c_int64, _vp, _vp, C.c_int32, _vp, _vp, _vp]),
    "c3dgs_debug_sort_temp_bytes": (C.c_size_t, [C.c_int32, C.c_int64, C.c_int32]),
    "c3dgs_debug_sort_pairs": (C.c_int, [C.c_int32, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "c3dgs_debug_tile_sort_temp_bytes": (C.c_size_t, [C.c_int32, C.c_int64]),
    "c3dgs_debug_tile_sort_pairs": (C.c_int, [C.c_int32, C.c_int64, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "c3dgs_debug_depth_plan": (C.c_int, [C.c_int32, C.c_uint32, C.c_int64, _vp, _vp, _vp]),
    "c3dgs_debug_depth_sort_temp_bytes": (C.c_size_t, [C.c_int64]),
    "c3dgs_debug_depth_sort": (C.c_int, [C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "c3dgs_get_geom_layout": (C.c_int, [C.c_int32, C.POINTER(GeomLayout)]),
    "c3dgs_get_binning_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(BinningLayout)]),
    "c3dgs_get_image_layout": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(ImageLayout)]),
    "c3dgs_get_compact_layout": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.POINTER(CompactLayout)]),
    "c3dgs_get_backward_layout": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(BackwardLayout)]),
    "c3dgs_backward_workspace_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "c3dgs_profile_enable": (C.c_int, [C.c_int]),
    "c3dgs_profile_only": (C.c_int, [C.c_char_p]),
    "c3dgs_profile_read": (C.c_int, [C.POINTER(StageTime), C.c_int]),
    "c3dgs_last_error": (C.c_char_p, []),
    "c3dgs_abi_version": (C.c_int, []),
    "c3dgs_abs_accumulate": (C.c_int, [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
}
# the measurement entries of include/c3dgs_hip_debug.h: only the diag variants of the library export them (build.py DIAG_VARIANTS)
DIAG_PROTOTYPES = {
    "c3dgs_debug_lane_counters": (C.c_int, [C.POINTER(C.c_uint64), _vp]),
    "c3dgs_debug_sort_times": (C.c_int, [C.POINTER(C.c_uint64)]),
    "c3dgs_debug_gather_probe": (C.c_int, [C.c_int32, C.c_int64, _vp, _vp, _vp, _vp]),
}

_lib = None


def lib():
    """Load the HIP library (once). Raises RuntimeError loudly when it is absent: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"c3dgs_amd: {LIB_PATH} is missing. Build it with `python -m c3dgs_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for this package.")
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as e:  # pragma: no cover
            raise RuntimeError(f"c3dgs_amd: cannot load {LIB_PATH}: {e}") from e
        diag = {n: p for n, p in DIAG_PROTOTYPES.items() if hasattr(handle, n)}
        for name, (res, args) in {**PROTOTYPES, **diag}.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc):
    if rc != 0:
        msg = lib().c3dgs_last_error()
        raise RuntimeError((msg or b"unknown error").decode("utf-8", "replace"))


# ---- the three things every caller of the library does with a torch tensor
def stream(device):
    """torch's current stream on `device`, as the library's stream argument."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def gpu_tensor(t, name, dtype=torch.float32):
    """`t` as the library reads it: contiguous, of `dtype`, on a GPU. Raises with `name` otherwise."""
    if not t.is_cuda:
        raise RuntimeError(f"c3dgs_amd: {name} must be a GPU tensor (there is no CPU path)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {str(dtype).split('.')[-1]}")
    return t.contiguous()


_workspaces = {}      # (key, device) -> the cached workspace (uint8), grown on demand


def workspace(key, device, nbytes, zeroed=False):
    """The workspace that module `key` ("optim", "mcmc") keeps per device: at least `nbytes`, reallocated (zero-filled if
    `zeroed`) only to grow, and 256-byte aligned as the library demands."""
    ws = _workspaces.get((key, device))
    if ws is None or ws.numel() < nbytes:
        ws = _workspaces[key, device] = (torch.zeros if zeroed else torch.empty)(nbytes, dtype=torch.uint8, device=device)
    if ws.data_ptr() % 256:
        raise RuntimeError(f"c3dgs_amd.{key}: the allocator returned a workspace that is not 256-byte aligned")
    return ws


def profile_enable(on=True, only=None):
    """Bracket stage launches with HIP events; `only` = one stage name to keep the queue cost to that kernel."""
    check(lib().c3dgs_profile_only(only.encode() if only else None))
    lib().c3dgs_profile_enable(1 if on else 0)


def profile_read():
    """-> {stage: (total_ms, count)} since the last read (synchronises the recorded events)."""
    arr = (StageTime * 64)()
    n = lib().c3dgs_profile_read(arr, 64)
    return {arr[i].name.decode(): (float(arr[i].total_ms), int(arr[i].count)) for i in range(n)}
